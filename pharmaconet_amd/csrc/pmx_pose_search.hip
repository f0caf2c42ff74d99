// pmx_pose_search.hip - pose search on gfx950: per hit, which of its conformers and binding modes to pose. pmx_pose_search takes the
// output of pmx_explain_modes, fits every (conformer, mode) slot of every hit with the library's own pmx_align, checks every fit with the
// library's own pmx_pose_clash, picks one slot per hit by the rule of include/pmx.h, and answers with what those two calls say about the
// chosen row. Everything between the two kernels of this unit lives in the caller's work buffer; tests/pose_search_ref.py restates the rule.
//
// expand_kernel - one wavefront per hit, kWaves per block, nothing shared between the waves of a block.
//   vbest     lanes over the hit's S = n_modes * conf_stride slots in trips of 64: the largest positive mode_max (a maximum: order-free)
//   rows      slot s = m * conf_stride + c becomes row i * S + s: the ligand, the key, and the conformer c - or -1 where the slot cannot
//             be a candidate whatever the fit says (the hit's status, v <= 0 or NaN, v < min_fraction * vbest). pmx_align and
//             pmx_pose_clash pass such a row through as PMX_LIGAND_KEY_INVALID without reading a coordinate.
// select_kernel - one wavefront per hit, the same lanes over the same slots.
//   lane      keeps the best of its slots under the order (passes, overlap ascending - 0 for a passing slot -, v descending, slot's
//             conformer ascending, mode ascending). The order is total over a hit's slots (no two share (c, m)), so
//   wave      the butterfly of __shfl_xor gives the same winner whatever its shape; the three counts are integer sums. No atomic.
// The chosen rows are then fitted and checked once more, n rows straight into the caller's outputs: a row's bits do not depend on where
// it stands in a call (include/pmx.h), so this is the gather, without a kernel that would have to know every output's layout.
// pmx_pose_search_atoms is the same sequence with the clash stage in point mode: pmx_atoms_gather (pmx_atoms.hip) makes the slots' rows of
// heavy atoms, merge_kernel hands a gather status that is not OK on to select_kernel, and the two kernels above run as they are.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "pmx.h"
#include "pmx_atoms.h" // struct pmx_atoms
#include "pmx_device.h"
#include "pmx_pose.h" // struct pmx_pocket

namespace {

constexpr int kWaves = 4;
constexpr int kC = PMX_MAX_CONFORMERS, kL = PMX_MAX_LEVELS, kN = PMX_MAX_LIGAND_NODES;
static_assert(kC == 64 && PMX_MAX_MODES * kC == 512, "a hit has at most 512 slots: eight trips of the lanes");

// The work buffer: the candidate rows, what pmx_align and pmx_pose_clash answer for them, and two arrays per hit.
struct Work {
    uint64_t *lig;      // [R]
    int32_t *conf;      // [R]
    uint8_t *key;       // [R][kL]
    double *rot;        // [R][9]
    double *trans;      // [R][3]
    double *fit;        // [R][8]
    double *node;       // [R][kN]
    int32_t *acount;    // [R][2]
    uint8_t *levels;    // [R][kL]
    int32_t *astatus;   // [R]
    double *summary;    // [R][4]
    int32_t *ccount;    // [R][6]
    double *pen;        // [R][kN]
    int32_t *atom;      // [R][kN]
    int32_t *cstatus;   // [R]
    double *vbest;      // [n]
    int32_t *chosen;    // [n] the chosen conformer (-1: none)
    // atom level only: the gathered rows (pen and atom are then [R * max_atoms], the layout of the points)
    int32_t *gstatus;   // [R]
    uint64_t *poff;     // [R + 1]
    float *points;      // [R * max_atoms][3]
    float *pradius;     // [R * max_atoms]
    uint64_t bytes;
};

// max_atoms < 0: the node-level search.
Work work_layout(void *base, uint64_t n, uint64_t R, int max_atoms = -1) {
    Work w{};
    uint64_t at = 0;
    auto take = [&](auto *&p, uint64_t count) {
        using T = std::remove_reference_t<decltype(*p)>;
        p = reinterpret_cast<T *>(reinterpret_cast<uintptr_t>(base) + at);
        at += (count * sizeof(T) + 255) & ~uint64_t(255);
    };
    take(w.lig, R);
    take(w.conf, R);
    take(w.key, R * kL);
    take(w.rot, R * 9);
    take(w.trans, R * 3);
    take(w.fit, R * 8);
    take(w.node, R * kN);
    take(w.acount, R * 2);
    take(w.levels, R * kL);
    take(w.astatus, R);
    take(w.summary, R * 4);
    take(w.ccount, R * 6);
    const uint64_t P = max_atoms < 0 ? R * kN : R * (uint64_t)max_atoms;
    take(w.pen, P);
    take(w.atom, P);
    take(w.cstatus, R);
    take(w.vbest, n);
    take(w.chosen, n);
    if (max_atoms >= 0) {
        take(w.gstatus, R);
        take(w.poff, R + 1);
        take(w.points, P * 3);
        take(w.pradius, P);
    }
    w.bytes = at + 256; // (never 0: a caller may always allocate what the query says)
    return w;
}

struct ExpandArgs {
    const uint64_t *ligands;
    const double *mode_max;
    const uint8_t *mode_match;
    const int32_t *estatus;
    uint32_t n;
    int n_modes, conf_stride;
    double min_fraction;
    uint64_t *lig;
    int32_t *conf;
    uint8_t *key;
    double *vbest;
};

__global__ __launch_bounds__(64 * kWaves) void expand_kernel(const ExpandArgs a) {
    const uint32_t hit = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (hit >= a.n) return;
    const int lane = (int)(threadIdx.x % 64);
    const int S = a.n_modes * a.conf_stride;
    const bool scored = a.estatus[hit] == PMX_LIGAND_OK;
    const uint64_t lig = a.ligands[hit];
    const size_t slot0 = (size_t)hit * a.n_modes; // (the hit's first [mode] block of mode_max)

    double vbest = 0.0;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        if (s < S) {
            const double v = a.mode_max[(slot0 + s / a.conf_stride) * kC + s % a.conf_stride];
            if (scored && v > vbest) vbest = v; // (a NaN never is)
        }
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        const double o = __shfl_xor(vbest, m);
        if (o > vbest) vbest = o;
    }
    const double floor_v = a.min_fraction * vbest;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        if (s >= S) continue;
        const int m = s / a.conf_stride, c = s % a.conf_stride;
        const size_t from = (slot0 + m) * kC + c, row = (size_t)hit * S + s;
        const double v = a.mode_max[from];
        a.lig[row] = lig;
        a.conf[row] = scored && v > 0.0 && v >= floor_v ? c : -1;
        for (int l = 0; l < kL; ++l) a.key[row * kL + l] = a.mode_match[from * kL + l];
    }
    if (lane == 0) a.vbest[hit] = vbest;
}

struct SelectArgs {
    const double *mode_max;
    const int32_t *estatus;
    uint32_t n;
    int n_modes, conf_stride, max_clashing, min_fitted;
    const int32_t *conf;
    const uint8_t *key;
    const int32_t *acount, *astatus;
    const double *summary;
    const int32_t *ccount, *cstatus;
    const double *vbest;
    int32_t *choice;
    double *value;
    uint8_t *key_out;
    int32_t *chosen;
    int32_t *status;
};

// One slot as the order sees it. s < 0: none.
struct Pick {
    int s, pass;
    double ov, v;
};

// Is x before y? (passes, overlap ascending, v descending, conformer ascending, mode ascending)
__device__ __forceinline__ bool before(const Pick &x, const Pick &y, int conf_stride) {
    if (x.s < 0) return false;
    if (y.s < 0) return true;
    if (x.pass != y.pass) return x.pass > y.pass;
    if (x.ov != y.ov) return x.ov < y.ov;
    if (x.v != y.v) return x.v > y.v;
    const int xc = x.s % conf_stride, yc = y.s % conf_stride;
    if (xc != yc) return xc < yc;
    return x.s < y.s; // (the same conformer: the lower mode)
}

__global__ __launch_bounds__(64 * kWaves) void select_kernel(const SelectArgs a) {
    const uint32_t hit = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (hit >= a.n) return;
    const int lane = (int)(threadIdx.x % 64);
    const int S = a.n_modes * a.conf_stride;
    const int est = a.estatus[hit];
    const size_t slot0 = (size_t)hit * a.n_modes;

    Pick best{-1, 0, 0.0, 0.0};
    int ncand = 0, npass = 0, ndrop = 0;
    for (int base = 0; base < S; base += 64) {
        const int s = base + lane;
        if (s >= S) continue;
        const size_t row = (size_t)hit * S + s;
        const double v = a.mode_max[(slot0 + s / a.conf_stride) * kC + s % a.conf_stride];
        if (a.conf[row] < 0) {
            ndrop += (int)(est == PMX_LIGAND_OK && v > 0.0); // (scored and positive: only the fraction can have taken it out)
            continue;
        }
        if (a.astatus[row] != PMX_LIGAND_OK || a.acount[row * 2] < a.min_fitted || a.cstatus[row] != PMX_LIGAND_OK) continue;
        Pick p;
        p.s = s;
        p.pass = (int)(a.ccount[row * 6 + 1] <= a.max_clashing);
        p.ov = p.pass ? 0.0 : a.summary[row * 4 + 1];
        p.v = v;
        ++ncand;
        npass += p.pass;
        if (before(p, best, a.conf_stride)) best = p;
    }
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
        Pick o;
        o.s = __shfl_xor(best.s, m);
        o.pass = __shfl_xor(best.pass, m);
        o.ov = __shfl_xor(best.ov, m);
        o.v = __shfl_xor(best.v, m);
        if (before(o, best, a.conf_stride)) best = o;
        ncand += __shfl_xor(ncand, m);
        npass += __shfl_xor(npass, m);
        ndrop += __shfl_xor(ndrop, m);
    }
    const bool any = best.s >= 0;
    const int c = any ? best.s % a.conf_stride : -1, m = any ? best.s / a.conf_stride : -1;
    if (lane < 6) a.choice[(size_t)hit * 6 + lane] = lane == 0 ? c : lane == 1 ? m : lane == 2 ? best.pass : lane == 3 ? ncand : lane == 4 ? npass : ndrop;
    if (lane < 2) a.value[(size_t)hit * 2 + lane] = !any ? __builtin_nan("") : lane == 0 ? best.v : best.v / a.vbest[hit];
    if (lane < kL) a.key_out[(size_t)hit * kL + lane] = any ? a.key[((size_t)hit * S + best.s) * kL + lane] : (uint8_t)0xFF;
    if (lane == 0) {
        a.chosen[hit] = c;
        a.status[hit] = est;
    }
}

// The atom-level search's one kernel of its own: a row whose gather status is not OK has no points, and pmx_pose_clash in point mode calls
// such a row valid (clearance -inf). It takes the gather's status, so that select_kernel skips it and a report says why.
__global__ __launch_bounds__(256) void merge_kernel(const int32_t *gstatus, int32_t *cstatus, uint32_t rows) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= rows) return;
    const int32_t g = gstatus[row];
    if (g != PMX_LIGAND_OK) cstatus[row] = g;
}

bool valid_shape(int n_modes, int conf_stride) { return n_modes >= 1 && n_modes <= PMX_MAX_MODES && conf_stride >= 1 && conf_stride <= PMX_MAX_CONFORMERS; }

} // namespace

extern "C" uint64_t pmx_pose_search_work_bytes(uint32_t n, int n_modes, int conf_stride) {
    if (!valid_shape(n_modes, conf_stride)) return 0;
    const uint64_t R = (uint64_t)n * (uint64_t)n_modes * (uint64_t)conf_stride;
    if (R > PMX_EXPLAIN_MAX) return 0;
    return work_layout(nullptr, n, R).bytes;
}

extern "C" int pmx_pose_search(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES], const double *node_center_dev, const pmx_pocket *pocket,
                               const uint64_t *ligands_dev, uint32_t n, const double *mode_max_dev, const uint8_t *mode_match_dev, const int32_t *explain_status_dev, int n_modes,
                               int conf_stride, float point_radius, float tolerance, float contact, int max_clashing, int min_fitted, double min_fraction, int32_t *choice_dev,
                               double *value_dev, uint8_t *key_dev, double *rot_dev, double *trans_dev, double *fit_dev, double *node_dev, int32_t *count_dev, uint8_t *levels_dev,
                               double *summary_dev, int32_t *clash_count_dev, double *point_pen_dev, int32_t *point_atom_dev, uint64_t *contact_fp_dev, int32_t *status_dev,
                               int32_t *row_status_dev, void *work_dev, uint64_t work_bytes, void *stream_) {
    if (!model || !lib || !weights || !pocket) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: null model, library, weights or pocket");
    if (n_modes < 1 || n_modes > PMX_MAX_MODES) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: n_modes %d outside 1 .. %d", n_modes, PMX_MAX_MODES);
    if (conf_stride < 1 || conf_stride > PMX_MAX_CONFORMERS) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: conf_stride %d outside 1 .. %d", conf_stride, PMX_MAX_CONFORMERS);
    if (!std::isfinite(point_radius) || !std::isfinite(tolerance) || !std::isfinite(contact)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: radius, tolerance and contact must be finite");
    if (max_clashing < 0 || min_fitted < 1) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: max_clashing %d must be >= 0 and min_fitted %d >= 1", max_clashing, min_fitted);
    if (!(min_fraction >= 0.0 && min_fraction <= 1.0)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: min_fraction %g outside [0, 1]", min_fraction);
    const uint64_t R = (uint64_t)n * (uint64_t)n_modes * (uint64_t)conf_stride;
    if (R > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: %llu rows (hits x modes x conformers), at most %d", (unsigned long long)R, PMX_EXPLAIN_MAX);
    if (n == 0) return PMX_OK;
    if (!node_center_dev || !ligands_dev || !mode_max_dev || !mode_match_dev || !explain_status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: null input");
    if (!choice_dev || !value_dev || !key_dev || !rot_dev || !trans_dev || !fit_dev || !node_dev || !count_dev || !levels_dev || !summary_dev || !clash_count_dev || !point_pen_dev ||
        !point_atom_dev || !contact_fp_dev || !status_dev || !row_status_dev)
        return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: null output");
    if (!work_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: null work buffer");
    const Work w = work_layout(work_dev, n, R);
    if (work_bytes < w.bytes) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: a work buffer of %llu bytes, %llu needed", (unsigned long long)work_bytes, (unsigned long long)w.bytes);
    if (reinterpret_cast<uintptr_t>(work_dev) % 16 != 0) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: the work buffer is not 16-byte aligned");
    const int device = lib->device;
    if (device != pocket->device) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search: the pocket is on device %d, the library on %d", pocket->device, device);
    PMX_HIPCHECK(hipSetDevice(device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid((n + kWaves - 1) / kWaves), block(64 * kWaves);

    const ExpandArgs e{ligands_dev, mode_max_dev, mode_match_dev, explain_status_dev, n, n_modes, conf_stride, min_fraction, w.lig, w.conf, w.key, w.vbest};
    expand_kernel<<<grid, block, 0, stream>>>(e);
    PMX_HIPCHECK(hipGetLastError());
    int rc = pmx_align(model, lib, weights, node_center_dev, w.lig, w.conf, w.key, (uint32_t)R, w.rot, w.trans, w.fit, w.node, w.acount, w.levels, w.astatus, stream_);
    if (rc != PMX_OK) return rc;
    rc = pmx_pose_clash(pocket, lib, w.lig, w.conf, nullptr, nullptr, nullptr, w.rot, w.trans, (uint32_t)R, point_radius, tolerance, contact, w.summary, w.ccount, w.pen, w.atom, nullptr,
                        w.cstatus, stream_);
    if (rc != PMX_OK) return rc;
    const SelectArgs s{mode_max_dev, explain_status_dev, n, n_modes, conf_stride, max_clashing, min_fitted, w.conf, w.key, w.acount, w.astatus, w.summary, w.ccount, w.cstatus, w.vbest,
                       choice_dev, value_dev, key_dev, w.chosen, status_dev};
    select_kernel<<<grid, block, 0, stream>>>(s);
    PMX_HIPCHECK(hipGetLastError());
    // the chosen rows, once more, into the caller's outputs
    rc = pmx_align(model, lib, weights, node_center_dev, ligands_dev, w.chosen, key_dev, n, rot_dev, trans_dev, fit_dev, node_dev, count_dev, levels_dev, row_status_dev, stream_);
    if (rc != PMX_OK) return rc;
    return pmx_pose_clash(pocket, lib, ligands_dev, w.chosen, nullptr, nullptr, nullptr, rot_dev, trans_dev, n, point_radius, tolerance, contact, summary_dev, clash_count_dev, point_pen_dev,
                          point_atom_dev, contact_fp_dev, row_status_dev + n, stream_);
}

extern "C" uint64_t pmx_pose_search_atoms_work_bytes(uint32_t n, int n_modes, int conf_stride, int max_atoms) {
    if (!valid_shape(n_modes, conf_stride) || max_atoms < 0 || max_atoms > PMX_MAX_LIGAND_ATOMS) return 0;
    const uint64_t R = (uint64_t)n * (uint64_t)n_modes * (uint64_t)conf_stride;
    if (R > PMX_EXPLAIN_MAX) return 0;
    return work_layout(nullptr, n, R, max_atoms).bytes;
}

extern "C" int pmx_pose_search_atoms(const pmx_model *model, const pmx_library *lib, const pmx_atoms *atoms, const float weights[PMX_NUM_TYPES], const double *node_center_dev,
                                     const pmx_pocket *pocket, const uint64_t *ligands_dev, uint32_t n, const double *mode_max_dev, const uint8_t *mode_match_dev,
                                     const int32_t *explain_status_dev, int n_modes, int conf_stride, float point_radius, float tolerance, float contact, int max_clashing,
                                     int min_fitted, double min_fraction, int32_t *choice_dev, double *value_dev, uint8_t *key_dev, double *rot_dev, double *trans_dev,
                                     double *fit_dev, double *node_dev, int32_t *count_dev, uint8_t *levels_dev, double *summary_dev, int32_t *clash_count_dev,
                                     uint64_t *point_off_dev, double *point_pen_dev, int32_t *point_atom_dev, uint64_t *contact_fp_dev, int32_t *status_dev, int32_t *row_status_dev,
                                     void *work_dev, uint64_t work_bytes, void *stream_) {
    if (!model || !lib || !atoms || !weights || !pocket) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: null model, library, atom store, weights or pocket");
    if (n_modes < 1 || n_modes > PMX_MAX_MODES) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: n_modes %d outside 1 .. %d", n_modes, PMX_MAX_MODES);
    if (conf_stride < 1 || conf_stride > PMX_MAX_CONFORMERS) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: conf_stride %d outside 1 .. %d", conf_stride, PMX_MAX_CONFORMERS);
    if (!std::isfinite(point_radius) || !std::isfinite(tolerance) || !std::isfinite(contact)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: radius, tolerance and contact must be finite");
    if (max_clashing < 0 || min_fitted < 1) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: max_clashing %d must be >= 0 and min_fitted %d >= 1", max_clashing, min_fitted);
    if (!(min_fraction >= 0.0 && min_fraction <= 1.0)) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: min_fraction %g outside [0, 1]", min_fraction);
    const uint64_t R = (uint64_t)n * (uint64_t)n_modes * (uint64_t)conf_stride;
    if (R > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: %llu rows (hits x modes x conformers), at most %d", (unsigned long long)R, PMX_EXPLAIN_MAX);
    if (n == 0) return PMX_OK;
    if (!node_center_dev || !ligands_dev || !mode_max_dev || !mode_match_dev || !explain_status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: null input");
    if (!choice_dev || !value_dev || !key_dev || !rot_dev || !trans_dev || !fit_dev || !node_dev || !count_dev || !levels_dev || !summary_dev || !clash_count_dev || !point_off_dev ||
        !point_pen_dev || !point_atom_dev || !contact_fp_dev || !status_dev || !row_status_dev)
        return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: null output");
    if (!work_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: null work buffer");
    const int max_atoms = atoms->info.max_atoms;
    const Work w = work_layout(work_dev, n, R, max_atoms);
    if (work_bytes < w.bytes) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: a work buffer of %llu bytes, %llu needed", (unsigned long long)work_bytes, (unsigned long long)w.bytes);
    if (reinterpret_cast<uintptr_t>(work_dev) % 16 != 0) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: the work buffer is not 16-byte aligned");
    const int device = lib->device;
    if (device != pocket->device) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: the pocket is on device %d, the library on %d", pocket->device, device);
    if (device != atoms->device) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_search_atoms: the atom store is on device %d, the library on %d", atoms->device, device);
    PMX_HIPCHECK(hipSetDevice(device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const dim3 grid((n + kWaves - 1) / kWaves), block(64 * kWaves);
    const uint64_t cap = R * (uint64_t)max_atoms; // (the chosen rows' n * max_atoms points fit the same buffers: n <= R)

    const ExpandArgs e{ligands_dev, mode_max_dev, mode_match_dev, explain_status_dev, n, n_modes, conf_stride, min_fraction, w.lig, w.conf, w.key, w.vbest};
    expand_kernel<<<grid, block, 0, stream>>>(e);
    PMX_HIPCHECK(hipGetLastError());
    int rc = pmx_align(model, lib, weights, node_center_dev, w.lig, w.conf, w.key, (uint32_t)R, w.rot, w.trans, w.fit, w.node, w.acount, w.levels, w.astatus, stream_);
    if (rc != PMX_OK) return rc;
    rc = pmx_atoms_gather(atoms, w.lig, w.conf, (uint32_t)R, cap, w.poff, w.points, w.pradius, w.gstatus, stream_);
    if (rc != PMX_OK) return rc;
    rc = pmx_pose_clash(pocket, nullptr, nullptr, nullptr, w.poff, w.points, w.pradius, w.rot, w.trans, (uint32_t)R, point_radius, tolerance, contact, w.summary, w.ccount, w.pen, w.atom,
                        nullptr, w.cstatus, stream_);
    if (rc != PMX_OK) return rc;
    merge_kernel<<<dim3(((uint32_t)R + 255) / 256), dim3(256), 0, stream>>>(w.gstatus, w.cstatus, (uint32_t)R);
    PMX_HIPCHECK(hipGetLastError());
    const SelectArgs s{mode_max_dev, explain_status_dev, n, n_modes, conf_stride, max_clashing, min_fitted, w.conf, w.key, w.acount, w.astatus, w.summary, w.ccount, w.cstatus, w.vbest,
                       choice_dev, value_dev, key_dev, w.chosen, status_dev};
    select_kernel<<<grid, block, 0, stream>>>(s);
    PMX_HIPCHECK(hipGetLastError());
    // the chosen rows, once more, into the caller's outputs (their points pass through the work buffer, which the slots no longer need)
    rc = pmx_align(model, lib, weights, node_center_dev, ligands_dev, w.chosen, key_dev, n, rot_dev, trans_dev, fit_dev, node_dev, count_dev, levels_dev, row_status_dev, stream_);
    if (rc != PMX_OK) return rc;
    rc = pmx_atoms_gather(atoms, ligands_dev, w.chosen, n, cap, point_off_dev, w.points, w.pradius, row_status_dev + n, stream_);
    if (rc != PMX_OK) return rc;
    rc = pmx_pose_clash(pocket, nullptr, nullptr, nullptr, point_off_dev, w.points, w.pradius, rot_dev, trans_dev, n, point_radius, tolerance, contact, summary_dev, clash_count_dev,
                        point_pen_dev, point_atom_dev, contact_fp_dev, row_status_dev + 2 * (size_t)n, stream_);
    if (rc != PMX_OK) return rc;
    merge_kernel<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(row_status_dev + n, row_status_dev + 2 * (size_t)n, n);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
