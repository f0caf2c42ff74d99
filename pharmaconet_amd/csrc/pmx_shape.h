// pmx_shape.h - what the two shape units share (pmx_pose_shape.hip: pmx_pose_shape, which judges a pose where it stands;
// pmx_shape_overlay.hip: pmx_shape_overlay and pmx_shape_starts, which move it), so that they cannot drift: the reference ligand's handle,
// the rules for a radius, and the pair term of include/pmx.h with the operations in the header's order.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"

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

} // namespace pmx
