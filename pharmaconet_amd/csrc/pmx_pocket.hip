// pmx_pocket.hip - excluded volumes on gfx950: pmx_pocket_create keeps the protein's atoms on the device, pmx_pose_clash checks posed
// rows - a library ligand's nodes, or any points of the caller's - against them: the deepest penetration, the overlap, the clashing and
// touching points, and the set of residues touched. The definitions are the comment of include/pmx.h; tests/clash_ref.py restates them.
//
// clash_kernel - one wavefront per row, kWaves per block, nothing shared between the waves of a block (no LDS array, no barrier).
//   points    a lane per point: point base + lane of the row, base = 0, 64, ... (a record has at most 64 nodes: one trip; a molecule's
//             atoms take as many as they need). The lane poses its point in float64 and keeps it in registers.
//   atoms     walked in index order, the same atom in every lane: the float4 (x, y, z, radius) and the group are read through addresses
//             that do not depend on the lane. The pocket is a few thousand float4, read-only, shared by every row: it stays in L2.
//   per pair  d2 first: an atom too far from every lane's point to change anything is passed over (see `lim2`); otherwise
//             d, pen in float64 as the header gives them. The lane keeps its point's largest pen with the first atom that attains it
//             (a strict >, atoms ascending), its clashing pairs, the sum of pen^2 in atom order, and whether it touches.
//   groups    the atom's group is a scalar; "some lane touches this atom" is a ballot, so the 256-bit set is four scalar words.
//   row       a lane adds up its points in ascending order; the lanes are combined by a butterfly of __shfl_xor whose shape is fixed,
//             the worst pair by the order (pen descending, point ascending). No atomic, no order that depends on timing.
// The other layout - the record's points x a slice of the atoms spread over the 64 lanes, and a reduction per point - is discussed with
// the measurement in DESIGN.md.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_pose.h" // struct pmx_pocket, the row front end, the posed point and the butterfly: shared with pmx_refine.hip

namespace {
using pmx::pose_load;
using pmx::pose_motion;
using pmx::pose_point;
using pmx::pose_row;
using pmx::PoseRow;
using pmx::PoseSource;
using pmx::wave_sum;

constexpr int kW = PMX_FINGERPRINT_WORDS;
constexpr int kN = PMX_MAX_LIGAND_NODES;
constexpr int kWaves = 4;
static_assert(kW == 4 && kN == 64, "a fingerprint is four words, a record's nodes take one trip of the lanes");

struct ClashArgs {
    const float4 *atoms;
    const uint16_t *group;
    uint32_t n_atoms;
    float max_radius;
    PoseSource src;
    const double *rot, *trans;
    uint32_t n;
    float radius, tolerance, contact;
    double *summary;
    int32_t *count;
    double *point_pen;
    int32_t *point_atom;
    uint64_t *fp;
    int32_t *status;
};

__global__ __launch_bounds__(64 * kWaves) void clash_kernel(const ClashArgs a) {
    // (everything a wavefront decides by is a scalar: its row, the record's header, the motion)
    const uint32_t row = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (row >= a.n) return;
    const int lane = (int)(threadIdx.x % 64);
    const double nan = __builtin_nan(""), ninf = -__builtin_inf();

    double R[9], t[3];
    const bool finite = pose_motion(a.rot, a.trans, row, R, t);

    // ---- the row's points
    const PoseRow pr = pose_row(a.src, row, finite);
    const int status = pr.status;
    const uint64_t out_at = pr.out_at;
    const uint32_t out_len = pr.out_len, npts = pr.npts;
    const float *radii = pr.radii;

    // ---- pairs
    const double tol = (double)a.tolerance, contact = (double)a.contact;
    double overlap = 0.0, best = ninf;
    int pairs = 0, clashing = 0, touching = 0, best_pt = -1, best_atom = -1;
    unsigned long long w0 = 0ull, w1 = 0ull, w2 = 0ull, w3 = 0ull;
    for (uint32_t base = 0; base < npts; base += 64) {
        const uint32_t u = base + (uint32_t)lane;
        const bool on = u < npts;
        double p0 = 0.0, p1 = 0.0, p2 = 0.0, rp = (double)a.radius;
        if (on) {
            double x0, x1, x2;
            pose_load(pr, u, x0, x1, x2);
            pose_point(R, t, x0, x1, x2, p0, p1, p2);
            if (radii) rp = (double)radii[u];
        }
        double pbest = ninf, pov = 0.0;
        int patom = -1, ppairs = 0;
        bool ptouch = false;
        // An atom at d > lim can neither touch (lim > contact), nor clash (lim > the largest contact sum smax), nor raise the point's largest
        // pen (pen <= smax - d < pbest), by a slack of 1e-6 that no rounding reaches: when that holds in every lane the atom is passed
        // over without its square root. Which atoms are passed over changes no output bit. lim is infinite until the point has a pen.
        const double smax = ((double)a.max_radius + rp) - tol;
        double lim2 = on ? -ninf : -1.0; // (a lane without a point never asks for an atom)
        for (uint32_t j = 0; j < a.n_atoms; ++j) {
            const float4 y = a.atoms[j];
            const double dx = p0 - (double)y.x, dy = p1 - (double)y.y, dz = p2 - (double)y.z;
            const double d2 = (dx * dx + dy * dy) + dz * dz;
            if (__ballot(d2 <= lim2) == 0ull) continue;
            const double d = __builtin_sqrt(d2);
            const double s = ((double)y.w + rp) - tol;
            const double pen = s - d;
            if (pen > pbest) {
                pbest = pen;
                patom = (int)j;
                if (on) {
                    const double lim = fmax(contact, smax - fmin(pbest, 0.0)) + 1e-6;
                    lim2 = lim * lim;
                }
            }
            if (pen > 0.0) {
                ++ppairs;
                pov += pen * pen;
            }
            const bool touch = on && d < contact;
            ptouch = ptouch || touch;
            if (a.fp && __ballot(touch) != 0ull) {
                const uint32_t g = a.group[j];
                const unsigned long long bit = 1ull << (g & 63u);
                w0 |= g < 64u ? bit : 0ull;
                w1 |= g >= 64u && g < 128u ? bit : 0ull;
                w2 |= g >= 128u && g < 192u ? bit : 0ull;
                w3 |= g >= 192u && g < 256u ? bit : 0ull;
            }
        }
        if (on) {
            a.point_pen[out_at + u] = pbest;
            a.point_atom[out_at + u] = patom;
            pairs += ppairs;
            clashing += (int)(ppairs > 0);
            touching += (int)ptouch;
            overlap += pov;
            if (pbest > best) { // (a lane's points ascend: the lowest point among equals stays)
                best = pbest;
                best_pt = (int)u;
                best_atom = patom;
            }
        }
    }
    // (what the loop did not write: the lanes beyond a record's nodes, every point of a row that is not OK)
    for (uint32_t u = npts + (uint32_t)lane; u < out_len; u += 64) {
        a.point_pen[out_at + u] = nan;
        a.point_atom[out_at + u] = -1;
    }

    // ---- the row
    pairs = wave_sum(pairs);
    clashing = wave_sum(clashing);
    touching = wave_sum(touching);
    overlap = wave_sum(overlap);
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double ob = __shfl_xor(best, m);
        const int op = __shfl_xor(best_pt, m), oa = __shfl_xor(best_atom, m);
        if (ob > best || (ob == best && op >= 0 && (best_pt < 0 || op < best_pt))) {
            best = ob;
            best_pt = op;
            best_atom = oa;
        }
    }
    const bool ok = status == PMX_LIGAND_OK;
    if (lane < 4) a.summary[(size_t)row * 4 + lane] = !ok ? nan : lane == 0 ? best : lane == 1 ? overlap : 0.0;
    if (lane < 6) {
        const int v = lane == 0 ? (int)npts : lane == 1 ? clashing : lane == 2 ? pairs : lane == 3 ? touching : lane == 4 ? best_pt : best_atom;
        a.count[(size_t)row * 6 + lane] = ok ? v : (lane < 4 ? 0 : -1);
    }
    if (a.fp && lane < kW) a.fp[(size_t)row * kW + lane] = lane == 0 ? w0 : lane == 1 ? w1 : lane == 2 ? w2 : w3;
    if (lane == 0) a.status[row] = status;
}

} // namespace

extern "C" int pmx_pocket_create(const float *xyz, const float *radius, const uint16_t *group, uint32_t n, int device, pmx_pocket **out) {
    if (!out) return pmx_fail(PMX_ERR_INVALID, "pmx_pocket_create: null out");
    *out = nullptr;
    if (n > PMX_POCKET_MAX_ATOMS) return pmx_fail(PMX_ERR_INVALID, "pmx_pocket_create: %u atoms, at most %d", n, PMX_POCKET_MAX_ATOMS);
    if (n > 0 && (!xyz || !radius)) return pmx_fail(PMX_ERR_INVALID, "pmx_pocket_create: null xyz or radius");
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_pocket_create: hipSetDevice failed");
    pmx_pocket *p = new pmx_pocket;
    p->device = device;
    p->n = n;
    if (n > 0) {
        std::vector<float4> atoms(n);
        std::vector<uint16_t> groups(n);
        for (uint32_t i = 0; i < n; ++i) {
            atoms[i] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], radius[i]);
            groups[i] = group ? group[i] : (uint16_t)0xFFFF;
            if (radius[i] > p->max_radius) p->max_radius = radius[i];
        }
        hipError_t e = hipMalloc(reinterpret_cast<void **>(&p->atoms), sizeof(float4) * n);
        if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&p->group), sizeof(uint16_t) * n);
        if (e == hipSuccess) e = hipMemcpy(p->atoms, atoms.data(), sizeof(float4) * n, hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMemcpy(p->group, groups.data(), sizeof(uint16_t) * n, hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            if (p->atoms) (void)hipFree(p->atoms);
            if (p->group) (void)hipFree(p->group);
            delete p;
            return pmx_fail(e == hipErrorOutOfMemory ? PMX_ERR_OOM : PMX_ERR_HIP, "pmx_pocket_create: %s", hipGetErrorString(e));
        }
    }
    *out = p;
    return PMX_OK;
}

extern "C" int pmx_pocket_destroy(pmx_pocket *pocket) {
    if (!pocket) return PMX_OK;
    if (pocket->atoms || pocket->group) {
        if (hipSetDevice(pocket->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_pocket_destroy: hipSetDevice failed");
        if (pocket->atoms) (void)hipFree(pocket->atoms);
        if (pocket->group) (void)hipFree(pocket->group);
    }
    delete pocket;
    return PMX_OK;
}

extern "C" int pmx_pose_clash(const pmx_pocket *pocket, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint64_t *point_off_dev,
                              const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev, uint32_t n, float point_radius,
                              float tolerance, float contact, double *summary_dev, int32_t *count_dev, double *point_pen_dev, int32_t *point_atom_dev, uint64_t *contact_fp_dev,
                              int32_t *status_dev, void *stream_) {
    ClashArgs a{};
    const int rc = pmx::pose_source("pmx_pose_clash", pocket, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, point_radius_dev, rot_dev, trans_dev, n, &a.src);
    if (rc != PMX_OK) return rc;
    if (!std::isfinite(point_radius) || !std::isfinite(tolerance) || !std::isfinite(contact)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_clash: radius, tolerance and contact must be finite");
    if (n == 0) return PMX_OK;
    if (!summary_dev || !count_dev || !point_pen_dev || !point_atom_dev || !status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_clash: null output (only contact_fp_dev may be)");
    if (hipSetDevice(pocket->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_pose_clash: hipSetDevice failed");
    a.atoms = pocket->atoms;
    a.group = pocket->group;
    a.n_atoms = pocket->n;
    a.max_radius = pocket->max_radius;
    a.rot = rot_dev;
    a.trans = trans_dev;
    a.n = n;
    a.radius = point_radius;
    a.tolerance = tolerance;
    a.contact = contact;
    a.summary = summary_dev;
    a.count = count_dev;
    a.point_pen = point_pen_dev;
    a.point_atom = point_atom_dev;
    a.fp = contact_fp_dev;
    a.status = status_dev;
    clash_kernel<<<dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, static_cast<hipStream_t>(stream_)>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
