// pmx_refine.hip - restrained rigid-body clash relief on gfx950: pmx_pose_refine moves each posed row - a library ligand's nodes, or any
// points of the caller's - out of the pocket's atoms by a bounded Levenberg-Marquardt minimisation over the six rigid degrees of freedom,
// held near where it started by a harmonic restraint on anchors. The definitions are the comment of include/pmx.h; tests/refine_ref.py
// restates them.
//
// refine_kernel - one wavefront per row, kWaves per block, nothing shared between the waves of a block (no LDS array, no barrier); each wave
// runs as many evaluations as its row takes.
//   evaluate   at a motion (R, t), three passes of the wave:
//     centroid   a lane per point in trips of 64, posed as pmx_pose_clash poses it; the lanes' sums are combined by the fixed butterfly
//     pairs      clash_kernel's walk: the same atom in every lane, d2 first, an atom that cannot clash with any lane's point is passed
//                over before its square root (the ballot). A clashing pair is rare: its 21 + 6 products are added under the lane mask
//     anchors    a lane per anchor, strided; the closed form of its block of H and g in r = q - c
//   reduce     Ec, Er, the pair count, H (21 values), g (6): one butterfly each - the same bits in every lane afterwards
//   iterate    pmx::lm_run of pmx_lm.h, the loop this call shares with pmx_shape_overlay, following E = Ec + restraint Er down
// H, g and the motions are named by constant indices only (every loop over them is unrolled): registers, no scratch.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_lm.h"
#include "pmx_pose.h"

namespace {
using pmx::hidx;
using pmx::lm_net_motion;
using pmx::lm_run;
using pmx::LmRun;
using pmx::pose_load;
using pmx::pose_motion;
using pmx::pose_point;
using pmx::pose_row;
using pmx::PoseRow;
using pmx::PoseSource;
using pmx::store_motion;
using pmx::store_not_ok;
using pmx::wave_sum;

constexpr int kWaves = 4;

struct RefineArgs {
    const float4 *atoms;
    uint32_t n_atoms;
    float max_radius;
    PoseSource src;
    const uint64_t *anchor_off; // null: the row's own points, each of weight 1
    const float *anchors;
    const double *anchor_target; // null: where the start motion puts the anchor
    const double *anchor_weight; // null: 1 each
    const double *rot, *trans;
    uint32_t n;
    float radius, tolerance;
    double restraint, ftol;
    int max_iter;
    double *rot_out, *trans_out, *energy;
    int32_t *count, *status;
};

struct Eval {
    double Ec, Er;
    int pairs;
    double c[3];
    double H[21], g[6];
};

struct Anchors {
    bool own;         // the row's own points
    uint32_t n;
    const float *xyz; // explicit anchors: xyz[3 k + .]
    const double *target, *weight;
};

__device__ __forceinline__ void evaluate(const RefineArgs &a, const PoseRow &pr, const Anchors &an, const double (&R0)[9], const double (&t0)[3], const double (&R)[9],
                                         const double (&t)[3], int lane, Eval &e) {
    const uint32_t npts = pr.npts;
    // ---- the centroid of the posed points
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        if (u < npts) {
            double x0, x1, x2, p0, p1, p2;
            pose_load(pr, u, x0, x1, x2);
            pose_point(R, t, x0, x1, x2, p0, p1, p2);
            s0 += p0;
            s1 += p1;
            s2 += p2;
        }
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    s2 = wave_sum(s2);
    const double c0 = npts ? s0 / (double)npts : 0.0, c1 = npts ? s1 / (double)npts : 0.0, c2 = npts ? s2 / (double)npts : 0.0;
    e.c[0] = c0;
    e.c[1] = c1;
    e.c[2] = c2;

    double H[21], g[6];
#pragma unroll
    for (int k = 0; k < 21; ++k) H[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 6; ++k) g[k] = 0.0;

    // ---- pairs
    const double tol = (double)a.tolerance;
    double overlap = 0.0;
    int pairs = 0;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        const bool on = u < npts;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, rp = (double)a.radius;
        if (on) {
            double x0, x1, x2;
            pose_load(pr, u, x0, x1, x2);
            pose_point(R, t, x0, x1, x2, p0, p1, p2);
            if (pr.radii) rp = (double)pr.radii[u];
        }
        const double r0 = p0 - c0, r1 = p1 - c1, r2 = p2 - c2;
        // A clashing pair has d < s <= smax, the largest contact sum of the point: an atom farther than smax, by a slack of 1e-6 that no
        // rounding reaches, from every lane's point is passed over without its square root. Which atoms are passed over changes no output bit.
        const double lim = (((double)a.max_radius + rp) - tol) + 1e-6;
        const double lim2 = on && lim > 0.0 ? lim * lim : -1.0; // (a lane without a point never asks for an atom)
        double pov = 0.0;
        int ppairs = 0;
        for (uint32_t j = 0; j < a.n_atoms; ++j) {
            const float4 y = a.atoms[j];
            const double dx = p0 - (double)y.x, dy = p1 - (double)y.y, dz = p2 - (double)y.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (__ballot(d2 <= lim2) == 0ull) continue;
            const double d = __builtin_sqrt(d2);
            const double s = ((double)y.w + rp) - tol;
            const double pen = s - d;
            if (on && pen > 0.0) {
                ++ppairs;
                pov += pen * pen;
                if (d > 0.0) {
                    double v[6];
                    v[3] = dx / d;
                    v[4] = dy / d;
                    v[5] = dz / d;
                    v[0] = r1 * v[5] - r2 * v[4];
                    v[1] = r2 * v[3] - r0 * v[5];
                    v[2] = r0 * v[4] - r1 * v[3];
#pragma unroll
                    for (int i = 0; i < 6; ++i) {
#pragma unroll
                        for (int k = i; k < 6; ++k) H[hidx(i, k)] += v[i] * v[k];
                        g[i] += -v[i] * pen;
                    }
                }
            }
        }
        if (on) {
            pairs += ppairs;
            overlap += pov;
        }
    }

    // ---- anchors
    double er = 0.0;
    for (uint32_t k = (uint32_t)lane; k < an.n; k += 64) {
        double x0, x1, x2, q0, q1, q2, b0, b1, b2;
        if (an.own) {
            pose_load(pr, k, x0, x1, x2);
        } else {
            x0 = (double)an.xyz[(size_t)k * 3];
            x1 = (double)an.xyz[(size_t)k * 3 + 1];
            x2 = (double)an.xyz[(size_t)k * 3 + 2];
        }
        pose_point(R, t, x0, x1, x2, q0, q1, q2);
        if (an.target) {
            b0 = an.target[(size_t)k * 3];
            b1 = an.target[(size_t)k * 3 + 1];
            b2 = an.target[(size_t)k * 3 + 2];
        } else {
            pose_point(R0, t0, x0, x1, x2, b0, b1, b2);
        }
        const double w = an.weight ? an.weight[k] : 1.0;
        const double kw = a.restraint * w;
        const double e0 = q0 - b0, e1 = q1 - b1, e2 = q2 - b2;
        const double r0 = q0 - c0, r1 = q1 - c1, r2 = q2 - c2;
        er += w * ((e0 * e0 + e1 * e1) + e2 * e2);
        const double rr = (r0 * r0 + r1 * r1) + r2 * r2;
        H[hidx(0, 0)] += kw * (rr - r0 * r0);
        H[hidx(0, 1)] += kw * -(r0 * r1);
        H[hidx(0, 2)] += kw * -(r0 * r2);
        H[hidx(1, 1)] += kw * (rr - r1 * r1);
        H[hidx(1, 2)] += kw * -(r1 * r2);
        H[hidx(2, 2)] += kw * (rr - r2 * r2);
        H[hidx(0, 4)] += kw * -r2;
        H[hidx(0, 5)] += kw * r1;
        H[hidx(1, 3)] += kw * r2;
        H[hidx(1, 5)] += kw * -r0;
        H[hidx(2, 3)] += kw * -r1;
        H[hidx(2, 4)] += kw * r0;
        H[hidx(3, 3)] += kw;
        H[hidx(4, 4)] += kw;
        H[hidx(5, 5)] += kw;
        g[0] += kw * (r1 * e2 - r2 * e1);
        g[1] += kw * (r2 * e0 - r0 * e2);
        g[2] += kw * (r0 * e1 - r1 * e0);
        g[3] += kw * e0;
        g[4] += kw * e1;
        g[5] += kw * e2;
    }

    // ---- the row
    e.pairs = wave_sum(pairs);
    e.Ec = wave_sum(overlap);
    e.Er = wave_sum(er);
#pragma unroll
    for (int k = 0; k < 21; ++k) e.H[k] = wave_sum(H[k]);
#pragma unroll
    for (int k = 0; k < 6; ++k) e.g[k] = wave_sum(g[k]);
}

// What pmx::lm_run follows: E = Ec + restraint Er, down.
struct Relief {
    using Eval = ::Eval;
    const RefineArgs &a;
    const PoseRow &pr;
    const Anchors &an;
    const double (&R0)[9], (&t0)[3];
    int lane;
    __device__ __forceinline__ void eval(const double (&R)[9], const double (&t)[3], Eval &e) const { evaluate(a, pr, an, R0, t0, R, t, lane, e); }
    __device__ __forceinline__ double value(const Eval &e) const { return e.Ec + a.restraint * e.Er; }
    __device__ __forceinline__ bool better(double trial, double cur) const { return trial < cur; }
    __device__ __forceinline__ double gain(double before, double after) const { return before - after; }
};

__global__ __launch_bounds__(64 * kWaves) void refine_kernel(const RefineArgs a) {
    const uint32_t row = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (row >= a.n) return;
    const int lane = (int)(threadIdx.x % 64);

    double R0[9], t0[3];
    const bool finite = pose_motion(a.rot, a.trans, row, R0, t0);
    const PoseRow pr = pose_row(a.src, row, finite);
    int status = pr.status;

    // ---- the anchors: the weights' sum, and a weight that is negative or not finite
    Anchors an;
    an.own = a.anchor_off == nullptr;
    double wsum = 0.0;
    if (an.own) {
        an.n = pr.npts;
        an.xyz = nullptr;
        an.target = an.weight = nullptr;
        wsum = (double)pr.npts;
    } else {
        const uint64_t o0 = a.anchor_off[row], o1 = a.anchor_off[row + 1];
        const uint64_t len = o1 > o0 ? o1 - o0 : 0ull;
        an.n = (uint32_t)(len < 0x7fffffffull ? len : 0x7fffffffull);
        an.xyz = a.anchors + o0 * 3;
        an.target = a.anchor_target ? a.anchor_target + o0 * 3 : nullptr;
        an.weight = a.anchor_weight ? a.anchor_weight + o0 : nullptr;
        bool bad = false;
        for (uint32_t k = (uint32_t)lane; k < an.n; k += 64) {
            const double w = an.weight ? an.weight[k] : 1.0;
            bad = bad || !(w >= 0.0) || !std::isfinite(w);
            wsum += w;
        }
        if (__ballot(bad) != 0ull && status == PMX_LIGAND_OK) status = PMX_LIGAND_KEY_INVALID;
        wsum = wave_sum(wsum);
    }

    if (status != PMX_LIGAND_OK) {
        store_not_ok<8, 4>(a.rot_out, a.trans_out, a.energy, a.count, a.status, row, lane, status);
        return;
    }

    // ---- the iteration, from the evaluation at the start; a row without a clashing pair has nothing to follow
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = t0[k];
    const Relief obj{a, pr, an, R0, t0, lane};
    Eval cur;
    obj.eval(R, t, cur);
    const double ec_start = cur.Ec, er_start = cur.Er;
    const double c_start[3] = {cur.c[0], cur.c[1], cur.c[2]};
    const LmRun run = lm_run(obj, cur, R, t, cur.pairs != 0, a.ftol, a.max_iter);

    // ---- the row's outputs: the last accepted motion (the input's own bits when nothing was accepted)
    double angle, shift;
    lm_net_motion(R, R0, run.accepted, cur.c, c_start, angle, shift);
    const double rmsd = wsum > 0.0 ? __builtin_sqrt(cur.Er / wsum) : 0.0;
    store_motion(a.rot_out, a.trans_out, row, lane, R, t);
    const double en[8] = {ec_start, er_start, cur.Ec, cur.Er, rmsd, angle, shift, run.lambda};
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) out = lane == k ? en[k] : out;
    if (lane < 8) a.energy[(size_t)row * 8 + lane] = out;
    if (lane < 4) a.count[(size_t)row * 4 + lane] = lane == 0 ? run.iterations : lane == 1 ? run.accepted : lane == 2 ? run.reason : cur.pairs;
    if (lane == 0) a.status[row] = status;
}

} // namespace

extern "C" int pmx_pose_refine(const pmx_pocket *pocket, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint64_t *point_off_dev,
                               const float *points_dev, const float *point_radius_dev, const uint64_t *anchor_off_dev, const float *anchors_dev,
                               const double *anchor_target_dev, const double *anchor_weight_dev, const double *rot_dev, const double *trans_dev, uint32_t n,
                               float point_radius, float tolerance, double restraint, double ftol, int max_iter, double *rot_out_dev, double *trans_out_dev,
                               double *energy_dev, int32_t *count_dev, int32_t *status_dev, void *stream_) {
    RefineArgs a{};
    const int rc = pmx::pose_source("pmx_pose_refine", pocket, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, point_radius_dev, rot_dev, trans_dev, n, &a.src);
    if (rc != PMX_OK) return rc;
    if (!std::isfinite(point_radius) || !std::isfinite(tolerance)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_refine: radius and tolerance must be finite");
    if (const int bad = pmx::lm_check("pmx_pose_refine", "restraint and ftol", ftol, max_iter, restraint)) return bad;
    if ((anchor_off_dev == nullptr) != (anchors_dev == nullptr)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_refine: anchor_off_dev and anchors_dev go together");
    if (!anchor_off_dev && (anchor_target_dev || anchor_weight_dev)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_refine: anchor targets or weights without anchors");
    if (n == 0) return PMX_OK;
    if (!rot_out_dev || !trans_out_dev || !energy_dev || !count_dev || !status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_refine: null output");
    if (hipSetDevice(pocket->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_pose_refine: hipSetDevice failed");
    a.atoms = pocket->atoms;
    a.n_atoms = pocket->n;
    a.max_radius = pocket->max_radius;
    a.anchor_off = anchor_off_dev;
    a.anchors = anchors_dev;
    a.anchor_target = anchor_target_dev;
    a.anchor_weight = anchor_weight_dev;
    a.rot = rot_dev;
    a.trans = trans_dev;
    a.n = n;
    a.radius = point_radius;
    a.tolerance = tolerance;
    a.restraint = restraint;
    a.ftol = ftol;
    a.max_iter = max_iter;
    a.rot_out = rot_out_dev;
    a.trans_out = trans_out_dev;
    a.energy = energy_dev;
    a.count = count_dev;
    a.status = status_dev;
    refine_kernel<<<dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, static_cast<hipStream_t>(stream_)>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
