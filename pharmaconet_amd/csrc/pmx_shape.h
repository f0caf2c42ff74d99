// pmx_shape.h - what the kernels that judge a row against a known ligand's Gaussian volume share, so that they cannot drift: shape_kernel
// (pmx_pose_shape.hip: pmx_pose_shape, which judges a pose where it stands), overlay_kernel (pmx_shape_overlay.hip: pmx_shape_overlay, which
// moves it) and combo_kernel (pmx_colour.hip: pmx_combo_overlay, which moves it by shape and colour together).
//   all three        the reference ligand's handle, the rules for a radius, the pair term of include/pmx.h with the operations in the
//                    header's order, the staging of the reference and of a row's shape points in LDS (stage_reference, stage_points),
//                    the self term O_AA (self_term; shape_kernel calls it inside its per-point loop) and the shape Tanimoto
//   shape, overlay   stage_shape_row: motion, pose_row, stage_points and the row's status in one. (combo_kernel's rows have a node source
//                    too; it merges the two statuses itself and ballots the radii with the masks. Given stage_shape_row and a ballot of
//                    its own, the compiler reloaded 32 spilled scalars per pair of its colour loop: 8 % of pmx_combo_overlay)
//   overlay, combo   self_overlap (the lanes' sums of self_term) and shape_evaluate, the evaluation the two iterate on
// pmx_shape_starts (starts_kernel) takes the handle alone.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"
#include "pmx_lm.h"   // hidx
#include "pmx_pose.h" // the posed point and the butterfly

struct pmx_shape_ref {
    int device = 0;
    uint32_t m = 0;
    double o_bb = 0.0;       // the reference's self-overlap: summary[1] of its own atoms as a row under the identity motion
    double4 *atoms = nullptr; // [m] y widened, alpha
};

namespace pmx {

constexpr double kShapeKappa = 2.4179879310247046;
constexpr double kShapePi = 3.141592653589793;

__host__ __device__ __forceinline__ bool radius_ok(float r) { return std::isfinite(r) && r > 0.0f; }
__host__ __device__ __forceinline__ double alpha_of(float r) { return kShapeKappa / ((double)r * (double)r); }

__device__ __forceinline__ double dist2(const double4 &p, const double4 &y) {
    const double e0 = p.x - y.x, e1 = p.y - y.y, e2 = p.z - y.z;
    return (e0 * e0 + e1 * e1) + e2 * e2;
}

// The pair term of include/pmx.h.
__device__ __forceinline__ double pair_term(double d2, double aa, double ab) {
    const double s = aa + ab;
    const double q = kShapePi / s;
    const double k = (aa * ab) / s;
    return (8.0 * (q * __builtin_sqrt(q))) * exp(-(k * d2));
}

// ... and with it the pair's k, which the overlay's gradient needs: the same operations, so V has pair_term's bits.
__device__ __forceinline__ double pair_term(double d2, double aa, double ab, double &k) {
    const double s = aa + ab;
    const double q = kShapePi / s;
    k = (aa * ab) / s;
    return (8.0 * (q * __builtin_sqrt(q))) * exp(-(k * d2));
}

__device__ __forceinline__ double tanimoto(double oab, double oaa, double obb) { return oab / ((oaa + obb) - oab); }

// ---- staging: a block of kShapeWaves wavefronts, a row each. The reference (y widened, alpha: 32 bytes an atom, at most 8 KB) is copied by
// the whole block, a row's points by its wavefront into its own slices. Neither function holds the barrier: the kernel has one
// __syncthreads() after its staging, which every wavefront of the block reaches - the ones beyond the call's last row and the ones whose
// row is not OK included. After it the LDS is only read.
constexpr int kShapeWaves = 4;

__device__ __forceinline__ void stage_reference(double4 *Lref, const double4 *ref, uint32_t m) {
    for (uint32_t b = threadIdx.x; b < m; b += 64 * kShapeWaves) Lref[b] = ref[b];
}

struct ShapeRow {
    int status;
    uint32_t npts; // 0 unless the status is PMX_LIGAND_OK
    PoseRow pr;
};

// The trips of a row's wavefront over its points: point u posed at (R0, t0) with its alpha into P[u] and - kUnposed - as it is, widened,
// with its alpha into X[u]. `radius` is the call's, for a source without radii of its own. Returns whether the lane met a radius that is
// none; the caller ballots it. At most PMX_MAX_LIGAND_ATOMS points: the caller has refused a longer row.
template <bool kUnposed>
__device__ __forceinline__ bool stage_points(const PoseRow &pr, uint32_t npts, const double (&R0)[9], const double (&t0)[3], float radius, int lane, double4 *P, double4 *X) {
    bool bad = false;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        if (u < npts) {
            double x0, x1, x2, p0, p1, p2;
            pose_load(pr, u, x0, x1, x2);
            pose_point(R0, t0, x0, x1, x2, p0, p1, p2);
            const float r = pr.radii ? pr.radii[u] : radius;
            bad = bad || !radius_ok(r);
            const double al = alpha_of(r);
            if (kUnposed) X[u] = make_double4(x0, x1, x2, al);
            P[u] = make_double4(p0, p1, p2, al);
        }
    }
    return bad;
}

// A row's shape points, from its motion to its status: the motion into (R0, t0), the row opened, its points staged (stage_points). The
// status is, in this order: a motion that is not finite or pose_row's own; PMX_LIGAND_UNSUPPORTED for more than PMX_MAX_LIGAND_ATOMS
// points (more than a molecule of the atom store can have: nothing of the row is staged); PMX_LIGAND_KEY_INVALID for a radius that is
// none. (combo_kernel, whose rows have a node source as well, merges the two sources' statuses itself and ballots the radii with the
// masks: it calls stage_points.)
template <bool kUnposed>
__device__ __forceinline__ ShapeRow stage_shape_row(const PoseSource &src, const double *rot, const double *trans, uint32_t row, float radius, int lane, double (&R0)[9],
                                                    double (&t0)[3], double4 *P, double4 *X) {
    ShapeRow s;
    const bool finite = pose_motion(rot, trans, row, R0, t0);
    s.pr = pose_row(src, row, finite);
    s.status = s.pr.status;
    s.npts = s.pr.npts;
    if (s.npts > (uint32_t)PMX_MAX_LIGAND_ATOMS) {
        s.status = PMX_LIGAND_UNSUPPORTED;
        s.npts = 0;
    }
    if (__ballot(stage_points<kUnposed>(s.pr, s.npts, R0, t0, radius, lane, P, X)) != 0ull) {
        s.status = PMX_LIGAND_KEY_INVALID;
        s.npts = 0;
    }
    return s;
}

// ---- O_AA of the staged points. self_a: point p against all points of the row in ascending a', itself included.
__device__ __forceinline__ double self_term(const double4 *P, uint32_t npts, const double4 &p) {
    double self = 0.0;
    for (uint32_t v = 0; v < npts; ++v) {
        const double4 q = P[v];
        self = self + pair_term(dist2(p, q), p.w, q.w);
    }
    return self;
}

// ... and the lane's sum of it over its points (base + lane, base = 0, 64, ...): O_AA is the butterfly of this, pmx_pose_shape's bits.
__device__ __forceinline__ double self_overlap(const double4 *P, uint32_t npts, int lane) {
    double sAA = 0.0;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        if (u < npts) sAA = sAA + self_term(P, npts, P[u]);
    }
    return sAA;
}

// ---- the evaluation pmx_shape_overlay and pmx_combo_overlay (pmx_colour.hip) iterate on: one definition, so that the two have the same bits
struct ShapeEval {
    double oab;
    double c[3];
    double H[21], g[6];
};

// O_AB, c, H and g at (R, t). X: the row's unposed points with their alphas; Lref: the reference.
__device__ __forceinline__ void shape_evaluate(const double4 *X, uint32_t npts, const double4 *Lref, uint32_t m, const double (&R)[9], const double (&t)[3], int lane, ShapeEval &e) {
    // ---- the centroid of the posed points
    double s0 = 0.0, s1 = 0.0, s2 = 0.0;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        if (u < npts) {
            const double4 x = X[u];
            double p0, p1, p2;
            pose_point(R, t, x.x, x.y, x.z, p0, p1, p2);
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

    // ---- pairs, and each point's block. (H(0,3), H(1,4), H(2,5), H(3,4), H(3,5) and H(4,5) are 0 by structure)
    double sAB = 0.0;
    double h00 = 0.0, h01 = 0.0, h02 = 0.0, h11 = 0.0, h12 = 0.0, h22 = 0.0, h04 = 0.0, h05 = 0.0, h13 = 0.0, h15 = 0.0, h23 = 0.0, h24 = 0.0, hw = 0.0;
    double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0, g5 = 0.0;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        if (u < npts) {
            const double4 x = X[u];
            double4 p;
            pose_point(R, t, x.x, x.y, x.z, p.x, p.y, p.z);
            p.w = x.w;
            double cross = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0, w = 0.0;
            for (uint32_t b = 0; b < m; ++b) {
                const double4 y = Lref[b];
                const double e0 = p.x - y.x, e1 = p.y - y.y, e2 = p.z - y.z;
                const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                double k;
                const double V = pair_term(d2, p.w, y.w, k);
                const double kappa = (2.0 * k) * V;
                cross = cross + V;
                f0 = f0 + kappa * e0;
                f1 = f1 + kappa * e1;
                f2 = f2 + kappa * e2;
                w = w + kappa;
            }
            sAB = sAB + cross;
            const double r0 = p.x - c0, r1 = p.y - c1, r2 = p.z - c2;
            const double rr = (r0 * r0 + r1 * r1) + r2 * r2;
            h00 += w * (rr - r0 * r0);
            h01 += w * -(r0 * r1);
            h02 += w * -(r0 * r2);
            h11 += w * (rr - r1 * r1);
            h12 += w * -(r1 * r2);
            h22 += w * (rr - r2 * r2);
            h04 += w * -r2;
            h05 += w * r1;
            h13 += w * r2;
            h15 += w * -r0;
            h23 += w * -r1;
            h24 += w * r0;
            hw += w;
            g0 += r1 * f2 - r2 * f1;
            g1 += r2 * f0 - r0 * f2;
            g2 += r0 * f1 - r1 * f0;
            g3 += f0;
            g4 += f1;
            g5 += f2;
        }
    }

    // ---- the row
    e.oab = wave_sum(sAB);
#pragma unroll
    for (int k = 0; k < 21; ++k) e.H[k] = 0.0;
    e.H[hidx(0, 0)] = wave_sum(h00);
    e.H[hidx(0, 1)] = wave_sum(h01);
    e.H[hidx(0, 2)] = wave_sum(h02);
    e.H[hidx(1, 1)] = wave_sum(h11);
    e.H[hidx(1, 2)] = wave_sum(h12);
    e.H[hidx(2, 2)] = wave_sum(h22);
    e.H[hidx(0, 4)] = wave_sum(h04);
    e.H[hidx(0, 5)] = wave_sum(h05);
    e.H[hidx(1, 3)] = wave_sum(h13);
    e.H[hidx(1, 5)] = wave_sum(h15);
    e.H[hidx(2, 3)] = wave_sum(h23);
    e.H[hidx(2, 4)] = wave_sum(h24);
    e.H[hidx(3, 3)] = e.H[hidx(4, 4)] = e.H[hidx(5, 5)] = wave_sum(hw);
    e.g[0] = wave_sum(g0);
    e.g[1] = wave_sum(g1);
    e.g[2] = wave_sum(g2);
    e.g[3] = wave_sum(g3);
    e.g[4] = wave_sum(g4);
    e.g[5] = wave_sum(g5);
}

} // namespace pmx
