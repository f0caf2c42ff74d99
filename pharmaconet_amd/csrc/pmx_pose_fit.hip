// pmx_pose_fit.hip - hotspot overlap of posed hits on gfx950: pmx_pose_fit says, for library ligands under given rigid motions, how well
// the posed ligand nodes sit on the model's hotspots - the Gaussian overlap of every (ligand node, model node) pair with the model node's
// radius as the positional sigma, the reference's weight * exp(-z^2 / 2), "passes" iff |z| < 2 and its majority rule per node, read in the
// pocket's frame. The definitions are the comment of include/pmx.h; tests/pose_fit_ref.py restates them.
//
// pose_fit_kernel<KEY> - one wavefront per row, kWaves per block, nothing shared between the waves of a block.
//   row       free mode: the row front end of pmx_pose.h (pmx_pose_clash's node mode); key mode: open_row of pmx_rows_front.h, pmx_align's,
//             in 512 bytes of LDS per wavefront - the only LDS of the kernel. Either way the status, the record and the conformer are scalars.
//   nodes     a lane per ligand node u: the lane poses its node in float64 (pose_point) and keeps it in registers.
//   hotspots  walked in index order, the same model node m in every lane: its type, weight, sigma and centre are read through addresses
//             that do not depend on the lane. "(u, m) is a pair" is a per-lane predicate: in free mode bit type(m) of u's type mask, in key
//             mode "m is the next entry of u's node subset" - the ascending list pmx_align walks, followed by a cursor per lane.
//   per pair  d2, z2, the pass and g as the header gives them. The lane adds g and w in ascending m - the specified order of node_fit -
//             and keeps its smallest z2 with the first m that attains it (a strict <).
//   per m     the smallest (z2, u) over the lanes by a butterfly of __shfl_xor under a total order, so its shape does not matter; lane m % 64
//             keeps the answer of node word m / 64 in registers and the row's 256 values leave in four coalesced stores. "Some lane passes"
//             is a ballot, so the occupied set is four scalar words.
//   row       the four sums by the fixed butterfly of pmx_pose.h (wave_sum), the counts as integer sums. No atomic of any kind.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#define PMX_NS pmx_f
#include "pmx_screen_tables.h" // ScreenParams, parse_record and the wavefront helpers open_row is written in (namespace pmx_f)
#include "pmx_rows_front.h"    // open_row, row_node_subset, row_status: the pairs of pmx_align
#include "pmx_pose.h"          // the node-mode row front end of pmx_pose_clash, the posed point, the fixed butterfly

namespace pmx_f {
using pmx::pose_load;
using pmx::pose_point;
using pmx::pose_row;
using pmx::PoseRow;
using pmx::PoseSource;
using pmx::wave_sum;

constexpr int kW = PMX_FINGERPRINT_WORDS;
constexpr int kWaves = 4;
static_assert(kW == 4 && kN == 64 && kW * 64 == PMX_MAX_MODEL_NODES, "a lane per ligand node; a lane per model node and node word");

struct FitArgs {
    const double *center, *sigma;
    const uint64_t *ligands;
    const int32_t *conformer;
    const uint8_t *key;
    const double *rot, *trans;
    uint32_t n;
    double *summary;
    int32_t *count;
    double *node_fit, *node_best, *node_z2;
    int32_t *node_target;
    double *hotspot_z2;
    int32_t *hotspot_node;
    uint64_t *fp;
    int32_t *status;
};

template <bool KEY>
__global__ __launch_bounds__(64 * kWaves) void pose_fit_kernel(const ScreenParams p, const FitArgs a) {
    __shared__ RowLds Ls[KEY ? kWaves : 1];
    // (everything a wavefront decides by is a scalar: its row, the record's header, the motion, the model node in hand)
    const int wave = uni((int)(threadIdx.x / 64));
    const uint32_t row = blockIdx.x * kWaves + (uint32_t)wave;
    if (row >= a.n) return;
    const int lane = (int)(threadIdx.x % 64);
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    double R[9], t[3];
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        R[k] = a.rot[(size_t)row * 9 + k];
        finite = finite && std::isfinite(R[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t[k] = a.trans[(size_t)row * 3 + k];
        finite = finite && std::isfinite(t[k]);
    }

    // ---- the row's nodes, and what says which model nodes pair with the lane's: its type mask (free mode) or its node subset (key mode)
    PoseRow pr;
    unsigned tm = 0u;
    uint32_t k = 0, k1 = 0;
    if (KEY) {
        RowLds &L = Ls[wave];
        const Rows rows{a.ligands, a.conformer, a.key, a.n, nullptr, nullptr, nullptr};
        const Row w = open_row(p, rows, L, row);
        pr.status = row_status(w, !finite);
        pr.node_mode = true;
        pr.out_at = (uint64_t)row * kN;
        pr.out_len = kN;
        pr.npts = pr.status == PMX_LIGAND_OK ? (uint32_t)w.n : 0u;
        pr.xyz = w.r.xyz + (pr.npts ? w.c : 0);
        pr.stride = (uint32_t)w.C;
        pr.radii = nullptr;
        if (pr.npts) {
            const uint32_t sid = row_node_subset(p, w, L, lane).sid; // (0 beyond the record and for a node outside the match list)
            if (sid != 0u) k = p.sub_off[sid], k1 = p.sub_off[sid + 1u];
        }
    } else {
        const PoseSource src{p.lib.offsets, p.lib.data, p.lib.n, a.ligands, a.conformer, nullptr, nullptr, nullptr};
        pr = pose_row(src, row, finite);
        if ((uint32_t)lane < pr.npts) tm = parse_record(p.lib.data + p.lib.offsets[a.ligands[row]]).typemask[lane] & 127u;
    }
    const int status = pr.status;
    const uint32_t npts = pr.npts;
    const bool on = (uint32_t)lane < npts;
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    if (on) {
        double x0, x1, x2;
        pose_load(pr, (uint32_t)lane, x0, x1, x2);
        pose_point(R, t, x0, x1, x2, p0, p1, p2);
    }

    // ---- pairs
    double sg = 0.0, sw = 0.0, bz = inf, bg = 0.0, bw = 0.0;
    int nu = 0, pu = 0, bm = -1;
    double hz[kW];
    int hn[kW];
    unsigned long long fpw[kW];
    const int Nm = npts ? p.M.Nm : 0; // (a row without nodes walks nothing)
#pragma unroll
    for (int j = 0; j < kW; ++j) {
        hz[j] = inf;
        hn[j] = -1;
        fpw[j] = 0ull;
        for (int mm = 0; mm < 64; ++mm) {
            const int m = 64 * j + mm;
            if (m >= Nm) break;
            const int ty = p.M.node_type[m];
            bool mem;
            if (KEY) {
                mem = k < k1 && (int)p.sub_nodes[k] == m;
                k += mem ? 1u : 0u;
            } else {
                mem = ((tm >> ty) & 1u) != 0u;
            }
            const double w = (double)p.W.w[ty], s = a.sigma[m];
            if (!(w > 0.0) || !(std::isfinite(s) && s > 0.0)) continue; // (no pair with this model node, in any lane)
            if (__ballot(mem) == 0ull) continue;
            const double e0 = p0 - a.center[3 * m], e1 = p1 - a.center[3 * m + 1], e2 = p2 - a.center[3 * m + 2];
            const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
            const double v = s * s;
            const double z2 = d2 / v;
            const bool pass = mem && d2 < 4.0 * v;
            const double g = w * exp(-0.5 * z2);
            if (mem) {
                sg = sg + g;
                sw = sw + w;
                if (nu == 0 || z2 < bz) { // (model nodes ascend: the lowest among equals stays)
                    bz = z2;
                    bm = m;
                    bg = g;
                    bw = w;
                }
                ++nu;
                pu += (int)pass;
            }
            fpw[j] |= __ballot(pass) != 0ull ? 1ull << mm : 0ull;
            // the smallest (z2, u) of this model node: a lane without the pair stands behind every lane with it
            double cz = mem ? z2 : inf;
            int cu = mem ? lane : -1;
#pragma unroll
            for (int x = 1; x < 64; x <<= 1) {
                const double oz = __shfl_xor(cz, x);
                const int ou = __shfl_xor(cu, x);
                if (ou >= 0 && (cu < 0 || oz < cz || (oz == cz && ou < cu))) {
                    cz = oz;
                    cu = ou;
                }
            }
            if (lane == mm) {
                hz[j] = cz;
                hn[j] = cu;
            }
        }
    }

    // ---- the nodes
    const bool ok = status == PMX_LIGAND_OK;
    const bool has = nu > 0;
    const double fit = has ? sg / (double)nu : 0.0, ideal = has ? sw / (double)nu : 0.0;
    {
        const size_t o = (size_t)row * kN + (size_t)lane;
        a.node_fit[o] = !ok ? nan : has ? fit : -1.0;
        a.node_best[o] = !ok ? nan : has ? bg : -1.0;
        a.node_z2[o] = !ok ? nan : has ? bz : -1.0;
        a.node_target[o] = has ? bm : -1;
    }
#pragma unroll
    for (int j = 0; j < kW; ++j) {
        const size_t o = (size_t)row * PMX_MAX_MODEL_NODES + (size_t)(64 * j + lane);
        a.hotspot_z2[o] = ok ? hz[j] : nan;
        a.hotspot_node[o] = hn[j];
    }

    // ---- the row
    const double s0 = wave_sum(fit), s1 = wave_sum(ideal), s2 = wave_sum(has ? bg : 0.0), s3 = wave_sum(has ? bw : 0.0);
    const int c0 = wave_sum((int)has), c1 = wave_sum(nu), c2 = wave_sum((int)(has && 2 * pu >= nu)), c3 = wave_sum(pu);
    if (lane < 4) {
        a.summary[(size_t)row * 4 + lane] = !ok ? nan : lane == 0 ? s0 : lane == 1 ? s1 : lane == 2 ? s2 : s3;
        a.count[(size_t)row * 4 + lane] = lane == 0 ? c0 : lane == 1 ? c1 : lane == 2 ? c2 : c3;
        a.fp[(size_t)row * kW + lane] = lane == 0 ? fpw[0] : lane == 1 ? fpw[1] : lane == 2 ? fpw[2] : fpw[3];
    }
    if (lane == 0) a.status[row] = status;
}

} // namespace pmx_f

extern "C" int pmx_pose_fit(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const double *node_center_dev, const double *node_sigma_dev,
                            const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint8_t *key_dev, const double *rot_dev, const double *trans_dev, uint32_t n,
                            double *summary_dev, int32_t *count_dev, double *node_fit_dev, double *node_best_dev, double *node_z2_dev, int32_t *node_target_dev,
                            double *hotspot_z2_dev, int32_t *hotspot_node_dev, uint64_t *occupied_fp_dev, int32_t *status_dev, void *stream_) {
    using namespace pmx_f;
    if (!model || !lib || !weights) return pmx_fail(PMX_ERR_INVALID, "null argument");
    if (model->device != lib->device) return pmx_fail(PMX_ERR_INVALID, "model and library live on different devices");
    if (n > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_fit: %u rows, at most %d", n, PMX_EXPLAIN_MAX);
    if (n == 0) return PMX_OK;
    if (!node_center_dev || !node_sigma_dev || !ligands_dev || !conformer_dev || !rot_dev || !trans_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_fit: null input (only key_dev may be)");
    if (!summary_dev || !count_dev || !node_fit_dev || !node_best_dev || !node_z2_dev || !node_target_dev || !hotspot_z2_dev || !hotspot_node_dev || !occupied_fp_dev || !status_dev)
        return pmx_fail(PMX_ERR_INVALID, "pmx_pose_fit: null output");
    PMX_HIPCHECK(hipSetDevice(lib->device));
    const ScreenParams p = row_params(model, lib, weights);
    const FitArgs a{node_center_dev, node_sigma_dev, ligands_dev, conformer_dev, key_dev, rot_dev, trans_dev, n, summary_dev, count_dev, node_fit_dev, node_best_dev, node_z2_dev,
                    node_target_dev, hotspot_z2_dev, hotspot_node_dev, occupied_fp_dev, status_dev};
    const dim3 grid((n + kWaves - 1) / kWaves), block(64 * kWaves);
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (key_dev) pose_fit_kernel<true><<<grid, block, 0, stream>>>(p, a);
    else pose_fit_kernel<false><<<grid, block, 0, stream>>>(p, a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
