// pmx_pose.h - what the kernels that pose a row's points under a rigid motion share, so that they cannot drift.
//   the pocket's handle       pmx_pocket.hip (pmx_pose_clash), pmx_refine.hip (pmx_pose_refine); pmx_pose_search.hip takes nothing else
//   the row front end         PoseSource, pose_motion, pose_row, pose_load: where a row's points come from and which status it has. The
//                             two pocket calls; pmx_pose_fit.hip; and through pmx_shape.h the calls against a reference ligand -
//                             pmx_pose_shape.hip, pmx_shape_overlay.hip, pmx_colour.hip
//   the posed point, the fixed butterfly   pose_point as include/pmx.h gives it, wave_sum: every unit above
//   the host's checks         pose_source, of the source and motion arguments the calls have in common: all of them but pmx_pose_fit
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_handles.h"

struct pmx_pocket {
    int device = 0;
    uint32_t n = 0;
    float max_radius = 0.0f;   // the largest of the radii (0 without atoms): what bounds a pair's contact sum
    float4 *atoms = nullptr;   // [n] x, y, z, radius
    uint16_t *group = nullptr; // [n]
};

namespace pmx {

// Where the rows of a call take their points from: the library's records (node mode) or the caller's points (point mode, lib_data null).
struct PoseSource {
    const uint64_t *lib_offsets; // node mode (null in point mode)
    const uint8_t *lib_data;
    uint64_t lib_n;
    const uint64_t *ligands;
    const int32_t *conformer;
    const uint64_t *point_off; // point mode
    const float *points;
    const float *point_radius;
};

// One row's points. Everything here is the same in every lane of the row's wavefront.
struct PoseRow {
    int status;
    bool node_mode;
    uint64_t out_at;    // where the row's per-point outputs begin
    uint32_t out_len;   // ... and how many there are
    uint32_t npts;      // 0 unless the status is PMX_LIGAND_OK
    const float *xyz;   // node mode: float k of node u at xyz[(3 u + k) * stride]; point mode: xyz[3 u + k]
    uint32_t stride;
    const float *radii; // per point, or null for the call's radius
};

// The row's motion: R and t loaded, and whether all 12 values are finite (what `pose_row` takes as `finite`).
__device__ __forceinline__ bool pose_motion(const double *rot, const double *trans, uint32_t row, double (&R)[9], double (&t)[3]) {
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
        R[k] = rot[(size_t)row * 9 + k];
        finite = finite && std::isfinite(R[k]);
    }
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        t[k] = trans[(size_t)row * 3 + k];
        finite = finite && std::isfinite(t[k]);
    }
    return finite;
}

// The row front end: `finite` says that the row's 12 motion values are.
__device__ __forceinline__ PoseRow pose_row(const PoseSource &a, uint32_t row, bool finite) {
    PoseRow r;
    r.node_mode = a.points == nullptr;
    r.status = finite ? PMX_LIGAND_OK : PMX_LIGAND_KEY_INVALID;
    r.npts = 0;
    r.xyz = nullptr;
    r.stride = 1;
    r.radii = nullptr;
    if (r.node_mode) {
        r.out_at = (uint64_t)row * PMX_MAX_LIGAND_NODES;
        r.out_len = PMX_MAX_LIGAND_NODES;
        const uint64_t lig = a.ligands[row];
        const int c = a.conformer[row];
        bool supported = lig < a.lib_n; // (not a ligand of the library: nothing is read)
        if (supported) {
            const Record rec = parse_record(a.lib_data + a.lib_offsets[lig]);
            supported = __builtin_amdgcn_readfirstlane((int)record_supported(rec)) != 0;
            const int C = __builtin_amdgcn_readfirstlane(rec.C);
            if (supported) {
                if (c < 0 || c >= C) {
                    r.status = PMX_LIGAND_KEY_INVALID;
                } else {
                    r.npts = (uint32_t)__builtin_amdgcn_readfirstlane(rec.n);
                    r.xyz = rec.xyz + c;
                    r.stride = (uint32_t)C;
                }
            }
        }
        if (!supported) r.status = PMX_LIGAND_UNSUPPORTED;
    } else {
        const uint64_t o0 = a.point_off[row], o1 = a.point_off[row + 1];
        const uint64_t len = o1 > o0 ? o1 - o0 : 0ull;
        r.out_at = o0;
        r.out_len = (uint32_t)(len < 0x7fffffffull ? len : 0x7fffffffull);
        r.npts = r.out_len;
        r.xyz = a.points + o0 * 3;
        r.radii = a.point_radius ? a.point_radius + o0 : nullptr;
    }
    if (r.status != PMX_LIGAND_OK) r.npts = 0;
    return r;
}

// Point u of the row, widened.
__device__ __forceinline__ void pose_load(const PoseRow &r, uint32_t u, double &x0, double &x1, double &x2) {
    const size_t at = r.node_mode ? (size_t)u * 3 * r.stride : (size_t)u * 3;
    const size_t step = r.node_mode ? r.stride : 1;
    x0 = (double)r.xyz[at];
    x1 = (double)r.xyz[at + step];
    x2 = (double)r.xyz[at + 2 * step];
}

// The posed point of include/pmx.h: p_k = ((R[k][0] x_0 + R[k][1] x_1) + R[k][2] x_2) + t_k, every operation rounded.
__device__ __forceinline__ void pose_point(const double (&R)[9], const double (&t)[3], double x0, double x1, double x2, double &p0, double &p1, double &p2) {
    p0 = ((R[0] * x0 + R[1] * x1) + R[2] * x2) + t[0];
    p1 = ((R[3] * x0 + R[4] * x1) + R[5] * x2) + t[1];
    p2 = ((R[6] * x0 + R[7] * x1) + R[8] * x2) + t[2];
}

__device__ __forceinline__ int wave_sum(int x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m);
    return x;
}

__device__ __forceinline__ double wave_sum(double x) {
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) x += __shfl_xor(x, m); // (a + b in both partners: the same bits in every lane, the same on every run)
    return x;
}

// Host: the checks the pose calls share - one source of points, the row count, the library's device - and the source itself. `fn` names
// the caller in the message, `owner` what the rows are judged against (the pocket, the reference) and `device` where that lives. `both`:
// the call also takes a library and points together (pmx_combo_overlay: the record's nodes carry the types, the points the shape) - the
// source then holds the two, and a copy of it with `points` null is the node-mode source of the same rows.
inline int pose_source(const char *fn, const char *owner, int device, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                       const uint64_t *point_off_dev, const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev, uint32_t n,
                       PoseSource *out, bool both = false) {
    const bool nodes = lib != nullptr, points = points_dev != nullptr || point_off_dev != nullptr || point_radius_dev != nullptr;
    if (nodes == points && !(both && nodes)) return pmx_fail(PMX_ERR_INVALID, "%s: %s", fn, nodes ? "a library and points: one source of points per call" : "neither a library nor points");
    if (n > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "%s: %u rows, at most %d", fn, n, PMX_EXPLAIN_MAX);
    *out = PoseSource{};
    if (nodes) {
        if (lib->device != device) return pmx_fail(PMX_ERR_INVALID, "%s: the %s is on device %d, the library on %d", fn, owner, device, lib->device);
        out->lib_offsets = lib->offsets;
        out->lib_data = lib->data;
        out->lib_n = lib->info.n_ligands;
    }
    if (n == 0) return PMX_OK;
    if (nodes ? (!ligands_dev || !conformer_dev) : (!point_off_dev || !points_dev)) return pmx_fail(PMX_ERR_INVALID, "%s: null %s", fn, nodes ? "ligands_dev or conformer_dev" : "point_off_dev or points_dev");
    if (nodes && points && (!point_off_dev || !points_dev)) return pmx_fail(PMX_ERR_INVALID, "%s: null point_off_dev or points_dev", fn);
    if (!rot_dev || !trans_dev) return pmx_fail(PMX_ERR_INVALID, "%s: null rot_dev or trans_dev", fn);
    out->ligands = ligands_dev;
    out->conformer = conformer_dev;
    out->point_off = point_off_dev;
    out->points = points_dev;
    out->point_radius = point_radius_dev;
    return PMX_OK;
}

// ... against a pocket: what pmx_pose_clash and pmx_pose_refine call.
inline int pose_source(const char *fn, const pmx_pocket *pocket, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                       const uint64_t *point_off_dev, const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev, uint32_t n,
                       PoseSource *out) {
    if (!pocket) return pmx_fail(PMX_ERR_INVALID, "%s: null pocket", fn);
    return pose_source(fn, "pocket", pocket->device, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, point_radius_dev, rot_dev, trans_dev, n, out);
}

} // namespace pmx
