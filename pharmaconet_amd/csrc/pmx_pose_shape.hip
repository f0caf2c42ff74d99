// pmx_pose_shape.hip - shape overlap of posed rows with a known ligand on gfx950: pmx_shape_ref_create keeps the reference ligand's atoms
// on the device, pmx_pose_shape says of posed rows - a library ligand's nodes, or any points of the caller's - how much of the reference's
// Gaussian volume they fill (Grant and Pickup's first-order overlap, the shape Tanimoto and the two Tversky fractions), how far each point
// is from the reference and each reference atom from the row, and the atom-for-atom RMSD where the two lists are one molecule's. The
// definitions are the comment of include/pmx.h; tests/shape_ref.py restates them.
//
// shape_kernel - one wavefront per row, kWaves per block.
//   LDS       the staging of pmx_shape.h (stage_reference, stage_shape_row without the unposed points): the reference, at most 8 KB, and
//             per wavefront its row's posed points with their alphas, at most 8 KB - 40 KB a block. The one barrier follows it.
//   points    a lane per point: point base + lane, base = 0, 64, 128, 192. The lane walks the reference in ascending b - every lane reads
//             the same address, a broadcast - for cross_a, near2_a and point_ref, then the row's points for self_a (pmx::self_term).
//   reference a lane per reference atom b walks the row's points in ascending a: ref_near2_b and ref_point are a per-lane minimum under a
//             strict <, so no minimum crosses lanes.
//   row       a lane adds up its points (its atoms) in ascending order; the lanes are combined by the fixed butterfly of pmx_pose.h.
// Every pair is evaluated - there is no cut-off by distance - so the sums are the specified ones. No atomic of any kind.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_pose.h"  // the row front end, the posed point, the butterfly and the host's checks: shared with pmx_pose_clash
#include "pmx_shape.h" // the reference's handle, the radius rules, the pair term, the staging and the self term: shared with the overlays

namespace {
using pmx::alpha_of;
using pmx::dist2;
using pmx::pair_term;
using pmx::PoseSource;
using pmx::radius_ok;
using pmx::self_term;
using pmx::ShapeRow;
using pmx::stage_shape_row;
using pmx::wave_sum;

constexpr int kA = PMX_MAX_LIGAND_ATOMS;
constexpr int kWaves = pmx::kShapeWaves;
static_assert(kA % 64 == 0 && PMX_MAX_LIGAND_NODES <= kA, "a row's points and the reference take whole trips of the lanes; a record's nodes fit");

struct ShapeArgs {
    const double4 *ref;
    uint32_t m;
    double o_bb;
    PoseSource src;
    const double *rot, *trans;
    uint32_t n;
    float radius, cover;
    double *summary;
    int32_t *count;
    double *point_near;
    int32_t *point_ref;
    double *ref_near;
    int32_t *ref_point;
    int32_t *status;
};

__global__ __launch_bounds__(64 * kWaves) void shape_kernel(const ShapeArgs a) {
    __shared__ double4 Lref[kA];
    __shared__ double4 Lpts[kWaves][kA];
    // (everything a wavefront decides by is a scalar: its row, the record's header, the motion)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const uint32_t row = blockIdx.x * kWaves + (uint32_t)wave;
    const bool live = row < a.n;
    const int lane = (int)(threadIdx.x % 64);
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    pmx::stage_reference(Lref, a.ref, a.m);

    // ---- the row's points, posed, with their alphas (pmx::stage_shape_row; the unposed points are not kept)
    ShapeRow sr{};
    double4 *P = Lpts[wave];
    if (live) {
        double R[9], t[3];
        sr = stage_shape_row<false>(a.src, a.rot, a.trans, row, a.radius, lane, R, t, P, nullptr);
    }
    __syncthreads();
    if (!live) return;
    const int status = sr.status;
    const uint32_t npts = sr.npts;
    const bool ok = status == PMX_LIGAND_OK;
    const uint64_t out_at = sr.pr.out_at;
    const uint32_t out_len = sr.pr.out_len, m = a.m;
    const double c2 = (double)a.cover * (double)a.cover;

    // ---- a lane per point: against the reference, then against the row itself
    const bool in_order = npts == m;
    double sAB = 0.0, sAA = 0.0, sA = 0.0, sO = 0.0;
    int covered = 0;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        if (u < npts) {
            const double4 p = P[u];
            double cross = 0.0, near2 = inf;
            int nb = -1;
            for (uint32_t b = 0; b < m; ++b) {
                const double4 y = Lref[b];
                const double d2 = dist2(p, y);
                cross = cross + pair_term(d2, p.w, y.w);
                if (nb < 0 || d2 < near2) { // (atoms ascend: the lowest among equals stays)
                    near2 = d2;
                    nb = (int)b;
                }
            }
            const double self = self_term(P, npts, p);
            a.point_near[out_at + u] = __builtin_sqrt(near2);
            a.point_ref[out_at + u] = nb;
            sAB = sAB + cross;
            sAA = sAA + self;
            sA = sA + near2;
            covered += (int)(near2 < c2);
            if (in_order) sO = sO + dist2(p, Lref[u]);
        }
    }
    // (what the loop did not write: the lanes beyond a record's nodes, every point of a row that is not OK)
    for (uint32_t u = npts + (uint32_t)lane; u < out_len; u += 64) {
        a.point_near[out_at + u] = nan;
        a.point_ref[out_at + u] = -1;
    }

    // ---- a lane per reference atom
    double sB = 0.0;
    int ref_covered = 0;
#pragma unroll
    for (uint32_t base = 0; base < (uint32_t)kA; base += 64) {
        const uint32_t b = base + (uint32_t)lane;
        double rn2 = inf;
        int rp = -1;
        if (ok && b < m) {
            const double4 y = Lref[b];
            for (uint32_t v = 0; v < npts; ++v) {
                const double d2 = dist2(P[v], y);
                if (rp < 0 || d2 < rn2) { // (points ascend: the lowest among equals stays)
                    rn2 = d2;
                    rp = (int)v;
                }
            }
            sB = sB + rn2;
            ref_covered += (int)(rn2 < c2);
        }
        const size_t o = (size_t)row * kA + b;
        a.ref_near[o] = ok ? __builtin_sqrt(rn2) : nan;
        a.ref_point[o] = rp;
    }

    // ---- the row
    const double oab = wave_sum(sAB), oaa = wave_sum(sAA), tA = wave_sum(sA), tB = wave_sum(sB), tO = wave_sum(sO);
    covered = wave_sum(covered);
    ref_covered = wave_sum(ref_covered);
    if (lane < 10) {
        const double obb = a.o_bb, dm = (double)m;
        double v = 0.0;
        if (lane == 0) v = oab;
        else if (lane == 1) v = oaa;
        else if (lane == 2) v = obb;
        else if (lane == 3) v = oab / ((oaa + obb) - oab);
        else if (lane == 4) v = oab / obb;
        else if (lane == 5) v = oaa == 0.0 ? 0.0 : oab / oaa;
        else if (lane == 6) v = npts ? __builtin_sqrt(tA / (double)npts) : nan;
        else if (lane == 7) v = __builtin_sqrt(tB / dm);
        else if (lane == 8) v = in_order ? __builtin_sqrt(tO / dm) : nan;
        a.summary[(size_t)row * 10 + lane] = ok ? v : nan;
    }
    if (lane < 4) {
        const int v = lane == 0 ? (int)npts : lane == 1 ? covered : lane == 2 ? ref_covered : (int)m;
        a.count[(size_t)row * 4 + lane] = ok ? v : 0;
    }
    if (lane == 0) a.status[row] = status;
}

void launch(const ShapeArgs &a, hipStream_t stream) { shape_kernel<<<dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream>>>(a); }

// O_BB: the reference's own float32 atoms and radii as one point-mode row under the identity motion, through the kernel every row takes.
hipError_t self_overlap(pmx_shape_ref *r, const float *xyz, const float *radius) {
    const uint32_t m = r->m;
    struct Fixed {
        double rot[9], trans[3], summary[10];
        uint64_t off[2];
        int32_t count[4], status[2];
    } fixed{};
    fixed.rot[0] = fixed.rot[4] = fixed.rot[8] = 1.0;
    fixed.off[1] = m;
    // one buffer: Fixed | point_near [m] | ref_near [kA] | xyz [3 m] | radius [m] | point_ref [m] | ref_point [kA]
    const size_t o_near = sizeof(Fixed), o_rnear = o_near + sizeof(double) * m, o_xyz = o_rnear + sizeof(double) * kA, o_rad = o_xyz + sizeof(float) * 3 * m,
                 o_pref = o_rad + sizeof(float) * m, o_rref = o_pref + sizeof(int32_t) * m, bytes = o_rref + sizeof(int32_t) * kA;
    char *buf = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&buf), bytes);
    if (e != hipSuccess) return e;
    e = hipMemcpy(buf, &fixed, sizeof(Fixed), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + o_xyz, xyz, sizeof(float) * 3 * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(buf + o_rad, radius, sizeof(float) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        Fixed *f = reinterpret_cast<Fixed *>(buf);
        ShapeArgs a{};
        a.ref = r->atoms;
        a.m = m;
        a.src.point_off = f->off;
        a.src.points = reinterpret_cast<const float *>(buf + o_xyz);
        a.src.point_radius = reinterpret_cast<const float *>(buf + o_rad);
        a.rot = f->rot;
        a.trans = f->trans;
        a.n = 1;
        a.summary = f->summary;
        a.count = f->count;
        a.point_near = reinterpret_cast<double *>(buf + o_near);
        a.point_ref = reinterpret_cast<int32_t *>(buf + o_pref);
        a.ref_near = reinterpret_cast<double *>(buf + o_rnear);
        a.ref_point = reinterpret_cast<int32_t *>(buf + o_rref);
        a.status = f->status;
        launch(a, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(&fixed, buf, sizeof(Fixed), hipMemcpyDeviceToHost); // (waits for the kernel)
    }
    (void)hipFree(buf);
    if (e == hipSuccess) r->o_bb = fixed.summary[1];
    return e;
}

} // namespace

extern "C" int pmx_shape_ref_create(const float *xyz, const float *radius, uint32_t m, int device, pmx_shape_ref **out) {
    if (!out) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_ref_create: null out");
    *out = nullptr;
    if (m < 1 || m > PMX_MAX_LIGAND_ATOMS) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_ref_create: %u atoms, 1 to %d", m, PMX_MAX_LIGAND_ATOMS);
    if (!xyz || !radius) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_ref_create: null xyz or radius");
    std::vector<double4> atoms(m);
    for (uint32_t i = 0; i < m; ++i) {
        if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2]))
            return pmx_fail(PMX_ERR_INVALID, "pmx_shape_ref_create: atom %u has a coordinate that is not finite", i);
        if (!radius_ok(radius[i])) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_ref_create: atom %u has a radius that is not a finite number > 0", i);
        atoms[i] = make_double4((double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], alpha_of(radius[i]));
    }
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_shape_ref_create: hipSetDevice failed");
    pmx_shape_ref *r = new pmx_shape_ref;
    r->device = device;
    r->m = m;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&r->atoms), sizeof(double4) * m);
    if (e == hipSuccess) e = hipMemcpy(r->atoms, atoms.data(), sizeof(double4) * m, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = self_overlap(r, xyz, radius);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (r->atoms) (void)hipFree(r->atoms);
        delete r;
        return pmx_fail(e == hipErrorOutOfMemory ? PMX_ERR_OOM : PMX_ERR_HIP, "pmx_shape_ref_create: %s", hipGetErrorString(e));
    }
    *out = r;
    return PMX_OK;
}

extern "C" int pmx_shape_ref_self(const pmx_shape_ref *ref, double *self_out) {
    if (!ref || !self_out) return pmx_fail(PMX_ERR_INVALID, "pmx_shape_ref_self: null argument");
    *self_out = ref->o_bb;
    return PMX_OK;
}

extern "C" int pmx_shape_ref_destroy(pmx_shape_ref *ref) {
    if (!ref) return PMX_OK;
    if (ref->atoms) {
        if (hipSetDevice(ref->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_shape_ref_destroy: hipSetDevice failed");
        (void)hipFree(ref->atoms);
    }
    delete ref;
    return PMX_OK;
}

extern "C" int pmx_pose_shape(const pmx_shape_ref *ref, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint64_t *point_off_dev,
                              const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev, uint32_t n, float point_radius,
                              float cover, double *summary_dev, int32_t *count_dev, double *point_near_dev, int32_t *point_ref_dev, double *ref_near_dev,
                              int32_t *ref_point_dev, int32_t *status_dev, void *stream_) {
    if (!ref) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_shape: null reference");
    ShapeArgs a{};
    const int rc = pmx::pose_source("pmx_pose_shape", "reference", ref->device, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, point_radius_dev, rot_dev, trans_dev, n,
                                    &a.src);
    if (rc != PMX_OK) return rc;
    if (!std::isfinite(point_radius) || !std::isfinite(cover) || cover < 0.0f) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_shape: point_radius and cover must be finite, cover >= 0");
    if (n == 0) return PMX_OK;
    if (!summary_dev || !count_dev || !point_near_dev || !point_ref_dev || !ref_near_dev || !ref_point_dev || !status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_shape: null output");
    if (hipSetDevice(ref->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_pose_shape: hipSetDevice failed");
    a.ref = ref->atoms;
    a.m = ref->m;
    a.o_bb = ref->o_bb;
    a.rot = rot_dev;
    a.trans = trans_dev;
    a.n = n;
    a.radius = point_radius;
    a.cover = cover;
    a.summary = summary_dev;
    a.count = count_dev;
    a.point_near = point_near_dev;
    a.point_ref = point_ref_dev;
    a.ref_near = ref_near_dev;
    a.ref_point = ref_point_dev;
    a.status = status_dev;
    launch(a, static_cast<hipStream_t>(stream_));
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
