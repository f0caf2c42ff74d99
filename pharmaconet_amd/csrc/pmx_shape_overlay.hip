// pmx_shape_overlay.hip - shape overlay on gfx950: pmx_shape_overlay moves each posed row - a library ligand's nodes, or any points of the
// caller's - by a bounded Levenberg-Marquardt maximisation of its Gaussian overlap O_AB with a known ligand over the six rigid degrees of
// freedom; pmx_shape_starts gives a row the four motions that lay its inertial frame on the reference's, so that an overlay need not start
// from a pose. The definitions are the comment of include/pmx.h; tests/overlay_ref.py restates them.
//
// overlay_kernel - one wavefront per row, kWaves per block.
//   LDS       the staging of pmx_shape.h (stage_reference, stage_shape_row): the reference, at most 8 KB, and per wavefront its row's
//             unposed points with their alphas (X, at most 8 KB) and the points posed at the input motion (P, at most 8 KB; read once,
//             for O_AA by pmx::self_overlap) - 72 KB a block. The one barrier follows it.
//   evaluate  pmx::shape_evaluate of pmx_shape.h at a motion (R, t), two passes of the wave over X:
//     centroid  a lane per point in trips of 64, posed as pmx_pose_clash poses it; the lanes' sums by the fixed butterfly
//     pairs     a lane per point walks the reference in ascending b - a broadcast read - for cross, f (3 values) and w: one exp and a
//               handful of multiply-adds a pair. The point's block of H (15 values that are not 0 by structure) and g (6) is formed once
//               per point, the closed form in r = p - c
//     reduce    O_AB, H, g: one butterfly each - the same bits in every lane afterwards
//   iterate   pmx::lm_run of pmx_lm.h, the loop this call shares with pmx_pose_refine and pmx_combo_overlay, following O_AB up
// H, g and the motions are named by constant indices only: registers, no scratch.
//
// starts_kernel - one wavefront per row, no LDS: the lanes' sums of the row's unposed points and of the reference's atoms, the butterfly,
// then the 3x3 Jacobi in every lane alike.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_lm.h"
#include "pmx_pose.h"
#include "pmx_shape.h"

namespace {
using pmx::lm_net_motion;
using pmx::lm_run;
using pmx::LmRun;
using pmx::pose_load;
using pmx::pose_row;
using pmx::PoseRow;
using pmx::PoseSource;
using pmx::ShapeRow;
using pmx::stage_shape_row;
using pmx::store_motion;
using pmx::store_not_ok;
using pmx::tanimoto;
using pmx::wave_sum;

constexpr int kA = PMX_MAX_LIGAND_ATOMS;
constexpr int kWaves = pmx::kShapeWaves;
static_assert(kA % 64 == 0 && PMX_MAX_LIGAND_NODES <= kA, "a row's points take whole trips of the lanes; a record's nodes fit");

struct OverlayArgs {
    const double4 *ref;
    uint32_t m;
    double o_bb;
    PoseSource src;
    const double *rot, *trans;
    uint32_t n;
    float radius;
    double ftol;
    int max_iter;
    double *rot_out, *trans_out, *energy;
    int32_t *count, *status;
};

struct StartsArgs {
    const double4 *ref;
    uint32_t m;
    PoseSource src;
    const int32_t *start;
    uint32_t n;
    double *rot_out, *trans_out, *frame;
    int32_t *status;
};

// What pmx::lm_run follows: O_AB, up. (E' < E, E = -O_AB)
struct Overlap {
    using Eval = pmx::ShapeEval;
    const double4 *X;
    uint32_t npts;
    const double4 *Lref;
    uint32_t m;
    int lane;
    __device__ __forceinline__ void eval(const double (&R)[9], const double (&t)[3], Eval &e) const { pmx::shape_evaluate(X, npts, Lref, m, R, t, lane, e); }
    __device__ __forceinline__ double value(const Eval &e) const { return e.oab; }
    __device__ __forceinline__ bool better(double trial, double cur) const { return trial > cur; }
    __device__ __forceinline__ double gain(double before, double after) const { return after - before; }
};

__global__ __launch_bounds__(64 * kWaves) void overlay_kernel(const OverlayArgs a) {
    __shared__ double4 Lref[kA];
    __shared__ double4 Lx[kWaves][kA];
    __shared__ double4 Lp[kWaves][kA];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const uint32_t row = blockIdx.x * kWaves + (uint32_t)wave;
    const bool live = row < a.n;
    const int lane = (int)(threadIdx.x % 64);

    pmx::stage_reference(Lref, a.ref, a.m);

    // ---- the row's points: unposed with their alphas, and posed at the input motion
    double R0[9], t0[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R0[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) t0[k] = 0.0;
    ShapeRow sr{};
    double4 *X = Lx[wave], *P = Lp[wave];
    if (live) sr = stage_shape_row<true>(a.src, a.rot, a.trans, row, a.radius, lane, R0, t0, P, X);
    __syncthreads();
    if (!live) return;
    const int status = sr.status;
    const uint32_t npts = sr.npts, m = a.m;

    if (status != PMX_LIGAND_OK) {
        store_not_ok<8, 4>(a.rot_out, a.trans_out, a.energy, a.count, a.status, row, lane, status);
        return;
    }

    // ---- O_AA, once, of the points posed at the input motion: pmx_pose_shape's terms in its order
    const double oaa = wave_sum(pmx::self_overlap(P, npts, lane));

    // ---- the iteration, from the evaluation at the start. No point, or a row so far away that every term underflows: nothing to follow
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = t0[k];
    const Overlap obj{X, npts, Lref, m, lane};
    pmx::ShapeEval cur;
    obj.eval(R, t, cur);
    const double o_start = cur.oab;
    const double c_start[3] = {cur.c[0], cur.c[1], cur.c[2]};
    const LmRun run = lm_run(obj, cur, R, t, npts != 0 && o_start > 0.0, a.ftol, a.max_iter);
    const double O = run.value;

    // ---- the row's outputs: the last accepted motion (the input's own bits when nothing was accepted)
    double angle, shift;
    lm_net_motion(R, R0, run.accepted, cur.c, c_start, angle, shift);
    store_motion(a.rot_out, a.trans_out, row, lane, R, t);
    const double obb = a.o_bb;
    const double en[8] = {o_start, O, oaa, obb, tanimoto(o_start, oaa, obb), tanimoto(O, oaa, obb), angle, shift};
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < 8; ++k) out = lane == k ? en[k] : out;
    if (lane < 8) a.energy[(size_t)row * 8 + lane] = out;
    if (lane < 4) a.count[(size_t)row * 4 + lane] = lane == 0 ? run.iterations : lane == 1 ? run.accepted : lane == 2 ? run.reason : (int)npts;
    if (lane == 0) a.status[row] = status;
}

// ---- inertial frames

struct Frame {
    double c[3];
    double ax[9]; // axis k at ax[3 k ..]
    double ev[3];
};

// The frame from a set's centre and its six sums of centred products (xx, xy, xz, yy, yz, zz): the cyclic Jacobi of include/pmx.h.
__device__ __forceinline__ void jacobi_frame(uint32_t count, double c0, double c1, double c2, const double (&S)[6], Frame &f) {
    double A[3][3] = {{S[0], S[1], S[2]}, {S[1], S[3], S[4]}, {S[2], S[4], S[5]}};
    double V[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    if (count < 1) {
#pragma unroll
        for (int i = 0; i < 3; ++i)
#pragma unroll
            for (int j = 0; j < 3; ++j) A[i][j] = 0.0;
        c0 = c1 = c2 = 0.0;
    }
#pragma unroll 1
    for (int sweep = 0; sweep < PMX_SHAPE_JACOBI_SWEEPS; ++sweep) {
#pragma unroll
        for (int pair = 0; pair < 3; ++pair) {
            const int p = pair == 2 ? 1 : 0, q = pair == 0 ? 1 : 2, r = 3 - p - q;
            const double apq = A[p][q];
            if (apq != 0.0) {
                const double app = A[p][p], aqq = A[q][q];
                const double theta = (aqq - app) / (2.0 * apq);
                const double at = __builtin_fabs(theta) + __builtin_sqrt(theta * theta + 1.0);
                const double tn = theta >= 0.0 ? 1.0 / at : -1.0 / at;
                const double cc = 1.0 / __builtin_sqrt(tn * tn + 1.0);
                const double ss = tn * cc;
                A[p][p] = app - tn * apq;
                A[q][q] = aqq + tn * apq;
                A[p][q] = A[q][p] = 0.0;
                const double arp = A[r][p], arq = A[r][q];
                A[r][p] = A[p][r] = cc * arp - ss * arq;
                A[r][q] = A[q][r] = ss * arp + cc * arq;
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = cc * vkp - ss * vkq;
                    V[k][q] = ss * vkp + cc * vkq;
                }
            }
        }
    }
    // descending eigenvalue, equal values keeping the lower index: the place of column i
    const double e0 = A[0][0], e1 = A[1][1], e2 = A[2][2];
    const int k0 = (int)(e1 > e0) + (int)(e2 > e0);
    const int k1 = (int)(e0 >= e1) + (int)(e2 > e1);
    // (column 2 takes the place that is left)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        // (selects, no indexing by a variable: registers)
#pragma unroll
        for (int j = 0; j < 3; ++j) f.ax[3 * k + j] = k0 == k ? V[j][0] : k1 == k ? V[j][1] : V[j][2];
        f.ev[k] = k0 == k ? e0 : k1 == k ? e1 : e2;
    }
    f.ax[6] = f.ax[1] * f.ax[5] - f.ax[2] * f.ax[4];
    f.ax[7] = f.ax[2] * f.ax[3] - f.ax[0] * f.ax[5];
    f.ax[8] = f.ax[0] * f.ax[4] - f.ax[1] * f.ax[3];
    f.c[0] = c0;
    f.c[1] = c1;
    f.c[2] = c2;
}

__global__ __launch_bounds__(64 * kWaves) void starts_kernel(const StartsArgs a) {
    const uint32_t row = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (row >= a.n) return;
    const int lane = (int)(threadIdx.x % 64);
    const double nan = __builtin_nan("");

    const PoseRow pr = pose_row(a.src, row, true);
    int status = pr.status;
    uint32_t npts = pr.npts;
    if (npts > (uint32_t)kA) {
        status = PMX_LIGAND_UNSUPPORTED;
        npts = 0;
    }
    const int start = a.start[row];
    if (status == PMX_LIGAND_OK && (start < 0 || start > 3)) status = PMX_LIGAND_KEY_INVALID;
    if (status != PMX_LIGAND_OK) {
        if (lane < 9) a.rot_out[(size_t)row * 9 + lane] = nan;
        if (lane < 3) a.trans_out[(size_t)row * 3 + lane] = nan;
        if (lane < 16) a.frame[(size_t)row * 16 + lane] = nan;
        if (lane == 0) a.status[row] = status;
        return;
    }

    // ---- the row's frame
    Frame fa, fb;
    {
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (uint32_t u = (uint32_t)lane; u < npts; u += 64) {
            double x0, x1, x2;
            pose_load(pr, u, x0, x1, x2);
            s0 += x0;
            s1 += x1;
            s2 += x2;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const double c0 = npts ? s0 / (double)npts : 0.0, c1 = npts ? s1 / (double)npts : 0.0, c2 = npts ? s2 / (double)npts : 0.0;
        double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t u = (uint32_t)lane; u < npts; u += 64) {
            double x0, x1, x2;
            pose_load(pr, u, x0, x1, x2);
            const double d0 = x0 - c0, d1 = x1 - c1, d2 = x2 - c2;
            S[0] += d0 * d0;
            S[1] += d0 * d1;
            S[2] += d0 * d2;
            S[3] += d1 * d1;
            S[4] += d1 * d2;
            S[5] += d2 * d2;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) S[k] = wave_sum(S[k]);
        jacobi_frame(npts, c0, c1, c2, S, fa);
    }
    // ---- the reference's
    {
        const uint32_t m = a.m;
        double s0 = 0.0, s1 = 0.0, s2 = 0.0;
        for (uint32_t b = (uint32_t)lane; b < m; b += 64) {
            const double4 y = a.ref[b];
            s0 += y.x;
            s1 += y.y;
            s2 += y.z;
        }
        s0 = wave_sum(s0);
        s1 = wave_sum(s1);
        s2 = wave_sum(s2);
        const double c0 = s0 / (double)m, c1 = s1 / (double)m, c2 = s2 / (double)m; // (a reference has at least one atom)
        double S[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (uint32_t b = (uint32_t)lane; b < m; b += 64) {
            const double4 y = a.ref[b];
            const double d0 = y.x - c0, d1 = y.y - c1, d2 = y.z - c2;
            S[0] += d0 * d0;
            S[1] += d0 * d1;
            S[2] += d0 * d2;
            S[3] += d1 * d1;
            S[4] += d1 * d2;
            S[5] += d2 * d2;
        }
#pragma unroll
        for (int k = 0; k < 6; ++k) S[k] = wave_sum(S[k]);
        jacobi_frame(m, c0, c1, c2, S, fb);
    }

    // ---- R = E_B D_s E_A^T, t = c_B - R c_A; D_0 = I, D_s the half turn about axis s - 1
    const double d0 = (start == 0 || start == 1) ? 1.0 : -1.0, d1 = (start == 0 || start == 2) ? 1.0 : -1.0, d2 = (start == 0 || start == 3) ? 1.0 : -1.0;
    double R[9], t[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (d0 * (fb.ax[i] * fa.ax[j]) + d1 * (fb.ax[3 + i] * fa.ax[3 + j])) + d2 * (fb.ax[6 + i] * fa.ax[6 + j]);
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) t[i] = fb.c[i] - ((R[3 * i] * fa.c[0] + R[3 * i + 1] * fa.c[1]) + R[3 * i + 2] * fa.c[2]);
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) out = lane == k ? R[k] : out;
    if (lane < 9) a.rot_out[(size_t)row * 9 + lane] = out;
#pragma unroll
    for (int k = 0; k < 3; ++k) out = lane == k ? t[k] : out;
    if (lane < 3) a.trans_out[(size_t)row * 3 + lane] = out;
    out = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) out = lane == k ? fa.c[k] : out;
#pragma unroll
    for (int k = 0; k < 9; ++k) out = lane == 3 + k ? fa.ax[k] : out;
#pragma unroll
    for (int k = 0; k < 3; ++k) out = lane == 12 + k ? fa.ev[k] : out;
    if (lane < 16) a.frame[(size_t)row * 16 + lane] = out;
    if (lane == 0) a.status[row] = status;
}

} // namespace

extern "C" int pmx_shape_overlay(const pmx_shape_ref *ref, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint64_t *point_off_dev,
                                 const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev, uint32_t n, float point_radius,
                                 double ftol, int max_iter, double *rot_out_dev, double *trans_out_dev, double *energy_dev, int32_t *count_dev, int32_t *status_dev,
                                 void *stream_) {
    if (!ref) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_overlay: null reference");
    OverlayArgs a{};
    const int rc = pmx::pose_source("pmx_shape_overlay", "reference", ref->device, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, point_radius_dev, rot_dev, trans_dev,
                                    n, &a.src);
    if (rc != PMX_OK) return rc;
    if (!std::isfinite(point_radius)) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_overlay: point_radius must be finite");
    if (const int bad = pmx::lm_check("pmx_shape_overlay", "ftol", ftol, max_iter)) return bad;
    if (n == 0) return PMX_OK;
    if (!rot_out_dev || !trans_out_dev || !energy_dev || !count_dev || !status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_overlay: null output");
    if (hipSetDevice(ref->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_shape_overlay: hipSetDevice failed");
    a.ref = ref->atoms;
    a.m = ref->m;
    a.o_bb = ref->o_bb;
    a.rot = rot_dev;
    a.trans = trans_dev;
    a.n = n;
    a.radius = point_radius;
    a.ftol = ftol;
    a.max_iter = max_iter;
    a.rot_out = rot_out_dev;
    a.trans_out = trans_out_dev;
    a.energy = energy_dev;
    a.count = count_dev;
    a.status = status_dev;
    overlay_kernel<<<dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, static_cast<hipStream_t>(stream_)>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_shape_starts(const pmx_shape_ref *ref, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint64_t *point_off_dev,
                                const float *points_dev, const int32_t *start_dev, uint32_t n, double *rot_out_dev, double *trans_out_dev, double *frame_dev,
                                int32_t *status_dev, void *stream_) {
    if (!ref) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_starts: null reference");
    if (n > 0 && n <= PMX_EXPLAIN_MAX && (!rot_out_dev || !trans_out_dev || !frame_dev || !status_dev)) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_starts: null output");
    StartsArgs a{};
    // (the call reads no motion: the two outputs stand in where the shared check asks for one)
    const int rc = pmx::pose_source("pmx_shape_starts", "reference", ref->device, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, nullptr, rot_out_dev, trans_out_dev, n,
                                    &a.src);
    if (rc != PMX_OK) return rc;
    if (n == 0) return PMX_OK;
    if (!start_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_starts: null start_dev");
    if (hipSetDevice(ref->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_shape_starts: hipSetDevice failed");
    a.ref = ref->atoms;
    a.m = ref->m;
    a.start = start_dev;
    a.n = n;
    a.rot_out = rot_out_dev;
    a.trans_out = trans_out_dev;
    a.frame = frame_dev;
    a.status = status_dev;
    starts_kernel<<<dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, static_cast<hipStream_t>(stream_)>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
