// pmx_colour.hip - colour overlap on gfx950: the typed counterpart of the two shape units. pmx_colour_ref_create keeps a known ligand's
// pharmacophore features (positions, 7-bit type masks, the type weights, one radius) on the device; pmx_pose_colour says of posed rows - a
// library ligand's nodes with the record's masks, or typed points of the caller's - how much of the reference's typed Gaussian overlap
// they reproduce where they stand; pmx_combo_overlay moves a row by shape and colour together, F = O_AB + colour_weight * C_AB, through
// the Levenberg-Marquardt loop of pmx_lm.h. The definitions are the comment of include/pmx.h; tests/colour_ref.py and tests/combo_ref.py
// restate them.
//
// Both kernels: one wavefront per row, kWaves per block, a lane per typed point of the row (a row has at most 64), kept in registers -
// another lane's point is read by a shuffle. The reference's features (32 bytes each) and masks (1 byte each) are staged in LDS once by
// the block, 2112 bytes; one barrier, after the staging, which every wavefront of the block reaches.
//
// colour_kernel
//   nodes     lane a walks the features in ascending b - a broadcast read - for its cross term, the per-type parts and its nearest typed
//             partner; then the row's nodes in ascending a' for its self term
//   features  lane b walks the row's nodes in ascending a: a per-lane minimum under a strict <
//   row       the lanes are combined by the fixed butterfly of pmx_pose.h; matched_fp is one ballot
// combo_kernel
//   LDS       overlay_kernel's 72 KB, staged by the same functions of pmx_shape.h (stage_reference; stage_points for the row's shape
//             points unposed and posed at the input; O_AA by pmx::self_overlap), and the features: 75840 bytes a block, two blocks a CU.
//             The kernel's own: the two sources' statuses, the node source's first, and the lane's node with its mask - a mask >= 128
//             goes through the one ballot the radii go through
//   evaluate  pmx::shape_evaluate of pmx_shape.h - the evaluation pmx_shape_overlay iterates on - then the colour pairs of the lane's
//             node: the same closed-form blocks with r = p - c, c the shape points' centroid; after the butterflies H = H_shape + cw *
//             H_colour and g likewise
//   iterate   pmx::lm_run, following F up
// H, g and the motions are named by constant indices only: registers, no scratch. What an evaluation leaves is the same in every lane, and
// the combo kernel hands it on in scalar registers (`scalar`): the two evaluations the loop holds cost no vector register, which keeps the
// kernel at two wavefronts a SIMD - the two blocks a CU its LDS allows. No atomic of any kind.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <vector>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_lm.h"
#include "pmx_pose.h"
#include "pmx_shape.h"

struct pmx_colour_ref {
    int device = 0;
    uint32_t f = 0;
    double alpha = 0.0;          // KAPPA / (r r): every feature and every typed point has the one radius
    double c_bb = 0.0;           // the reference's self-overlap: summary[1] of its own features as a row under the identity motion
    double w[PMX_NUM_TYPES] = {}; // the type weights, widened
    double4 *feat = nullptr;     // [f] y widened (w: 0)
    uint8_t *mask = nullptr;     // [f], in the allocation of `feat`
};

namespace {
using pmx::dist2;
using pmx::hidx;
using pmx::lm_net_motion;
using pmx::lm_run;
using pmx::LmRun;
using pmx::pair_term;
using pmx::pose_load;
using pmx::pose_motion;
using pmx::pose_point;
using pmx::pose_row;
using pmx::PoseRow;
using pmx::PoseSource;
using pmx::radius_ok;
using pmx::ShapeEval;
using pmx::store_motion;
using pmx::store_not_ok;
using pmx::tanimoto;
using pmx::wave_sum;

constexpr int kA = PMX_MAX_LIGAND_ATOMS;
constexpr int kF = PMX_MAX_LIGAND_NODES; // typed points of a row, features of a reference: a lane each
constexpr int kT = PMX_NUM_TYPES;
constexpr int kWaves = pmx::kShapeWaves;
static_assert(kF == 64, "a lane per typed point and per feature: one trip of the wavefront");
static_assert(kT == 7, "a type mask is 7 bits: < 128");

// What a kernel reads of the colour reference.
struct ColourRef {
    const double4 *feat;
    const uint8_t *mask;
    uint32_t f;
    double alpha, c_bb;
    double w[kT];
};

ColourRef colour_ref_args(const pmx_colour_ref *r) {
    ColourRef c{};
    c.feat = r->feat;
    c.mask = r->mask;
    c.f = r->f;
    c.alpha = r->alpha;
    c.c_bb = r->c_bb;
    for (int t = 0; t < kT; ++t) c.w[t] = r->w[t];
    return c;
}

// The weight of a pair whose masks share the bits `shared`: the weights of those types, added in ascending type. (A type that is not
// shared adds 0.0, which changes no bit of a sum that is not negative.)
__device__ __forceinline__ double pair_weight(uint32_t shared, const ColourRef &c) {
    double w = 0.0;
#pragma unroll
    for (int t = 0; t < kT; ++t) w = w + (((shared >> t) & 1u) ? c.w[t] : 0.0);
    return w;
}

__device__ __forceinline__ void stage_features(const ColourRef &c, double4 *Lfeat, uint8_t *Lmask) {
    if (threadIdx.x < c.f) {
        Lfeat[threadIdx.x] = c.feat[threadIdx.x];
        Lmask[threadIdx.x] = c.mask[threadIdx.x];
    }
}

// The masks of a node-mode row that is OK: the record's.
__device__ __forceinline__ const uint8_t *record_masks(const PoseSource &s, uint32_t row) { return pmx::parse_record(s.lib_data + s.lib_offsets[s.ligands[row]]).typemask; }

// self_a: the lane's posed node p with mask mk (lanes >= nn hold nothing) against all nodes of the row in ascending a', itself included.
__device__ __forceinline__ double colour_self(double p0, double p1, double p2, uint32_t mk, uint32_t nn, int lane, const ColourRef &c) {
    double self = 0.0;
    for (uint32_t v = 0; v < nn; ++v) {
        const double q0 = __shfl(p0, (int)v), q1 = __shfl(p1, (int)v), q2 = __shfl(p2, (int)v);
        const uint32_t mv = (uint32_t)__shfl((int)mk, (int)v);
        const double w = pair_weight(mk & mv, c);
        if ((uint32_t)lane < nn && w != 0.0) {
            const double e0 = p0 - q0, e1 = p1 - q1, e2 = p2 - q2;
            const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
            self = self + w * pair_term(d2, c.alpha, c.alpha);
        }
    }
    return self;
}

// A value every lane holds alike (the result of a butterfly), moved to scalar registers: what a row keeps across the whole iteration costs
// no vector register there.
__device__ __forceinline__ double scalar(double x) {
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)u), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

__device__ __forceinline__ double colour_tanimoto(double cab, double caa, double cbb) { return cab == 0.0 ? 0.0 : cab / ((caa + cbb) - cab); }

// ---------------------------------------------------------------------------------------------------------------- pmx_pose_colour
struct ColourArgs {
    ColourRef ref;
    PoseSource src;
    const uint8_t *feat_mask; // feature mode: the masks of the caller's points, in the layout of the points
    const double *rot, *trans;
    uint32_t n;
    float cover;
    double *summary, *type_overlap;
    int32_t *count;
    double *node_colour, *node_near;
    int32_t *node_feature;
    double *feat_near;
    int32_t *feat_node;
    uint64_t *matched_fp;
    int32_t *status;
};

__global__ __launch_bounds__(64 * kWaves) void colour_kernel(const ColourArgs a) {
    __shared__ double4 Lfeat[kF];
    __shared__ uint8_t Lmask[kF];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const uint32_t row = blockIdx.x * kWaves + (uint32_t)wave;
    const int lane = (int)(threadIdx.x % 64);
    const double nan = __builtin_nan(""), inf = __builtin_inf();
    stage_features(a.ref, Lfeat, Lmask);
    __syncthreads();
    if (row >= a.n) return;

    // ---- the row's typed points: the lane's own, posed
    double R[9], t[3];
    const bool finite = pose_motion(a.rot, a.trans, row, R, t);
    const PoseRow pr = pose_row(a.src, row, finite);
    int status = pr.status;
    uint32_t nn = pr.npts;
    if (nn > (uint32_t)kF) { // (feature mode: more typed points than a record has nodes)
        status = PMX_LIGAND_UNSUPPORTED;
        nn = 0;
    }
    double p0 = 0.0, p1 = 0.0, p2 = 0.0;
    uint32_t mk = 0;
    if (nn) {
        const uint8_t *masks = pr.node_mode ? record_masks(a.src, row) : a.feat_mask + pr.out_at;
        bool bad = false;
        if ((uint32_t)lane < nn) {
            double x0, x1, x2;
            pose_load(pr, (uint32_t)lane, x0, x1, x2);
            pose_point(R, t, x0, x1, x2, p0, p1, p2);
            mk = masks[lane];
            bad = mk >= 128u;
        }
        if (__ballot(bad) != 0ull) {
            status = PMX_LIGAND_KEY_INVALID;
            nn = 0;
            mk = 0;
        }
    }
    const bool ok = status == PMX_LIGAND_OK;
    const bool mine = (uint32_t)lane < nn;
    const uint32_t f = a.ref.f;
    const double al = a.ref.alpha;
    const double c2 = (double)a.cover * (double)a.cover;

    // ---- a lane per node: against the features, then against the row itself
    double cross = 0.0, near2 = inf;
    int nb = -1;
    double ct[kT];
#pragma unroll
    for (int k = 0; k < kT; ++k) ct[k] = 0.0;
    if (mine) {
        const double4 p = make_double4(p0, p1, p2, 0.0);
        for (uint32_t b = 0; b < f; ++b) {
            const uint32_t shared = mk & (uint32_t)Lmask[b];
            const double w = pair_weight(shared, a.ref);
            if (w != 0.0) {
                const double d2 = dist2(p, Lfeat[b]);
                const double V = pair_term(d2, al, al);
                cross = cross + w * V;
#pragma unroll
                for (int k = 0; k < kT; ++k)
                    if ((shared >> k) & 1u) ct[k] = ct[k] + a.ref.w[k] * V;
                if (nb < 0 || d2 < near2) { // (features ascend: the lowest among equals stays)
                    near2 = d2;
                    nb = (int)b;
                }
            }
        }
    }
    const double self = colour_self(p0, p1, p2, mk, nn, lane, a.ref);

    // ---- a lane per feature
    double fn2 = inf;
    int fa = -1;
    {
        const bool feature = ok && (uint32_t)lane < f;
        const double4 y = feature ? Lfeat[lane] : make_double4(0.0, 0.0, 0.0, 0.0);
        const uint32_t mb = feature ? (uint32_t)Lmask[lane] : 0u;
        for (uint32_t v = 0; v < nn; ++v) {
            const double4 q = make_double4(__shfl(p0, (int)v), __shfl(p1, (int)v), __shfl(p2, (int)v), 0.0);
            const uint32_t mv = (uint32_t)__shfl((int)mk, (int)v);
            if (feature && pair_weight(mv & mb, a.ref) != 0.0) {
                const double d2 = dist2(q, y); // (p - y, as on the other side: the same bits)
                if (fa < 0 || d2 < fn2) {
                    fn2 = d2;
                    fa = (int)v;
                }
            }
        }
    }

    // ---- per node, per feature
    {
        const size_t o = (size_t)row * kF + lane;
        const bool paired = nb >= 0;
        a.node_colour[o] = mine ? cross : nan;
        a.node_near[o] = paired ? __builtin_sqrt(near2) : nan;
        a.node_feature[o] = nb;
        a.feat_near[o] = fa >= 0 ? __builtin_sqrt(fn2) : nan;
        a.feat_node[o] = fa;
    }

    // ---- the row
    const double cab = wave_sum(cross), caa = wave_sum(self), tA = wave_sum(nb >= 0 ? near2 : 0.0);
    const int matched = wave_sum((int)(nb >= 0)), covered = wave_sum((int)(nb >= 0 && near2 < c2));
    const uint64_t fp = __ballot(fa >= 0 && fn2 < c2);
    const int ref_covered = __popcll(fp);
#pragma unroll
    for (int k = 0; k < kT; ++k) ct[k] = wave_sum(ct[k]);
    if (lane < 8) {
        const double cbb = a.ref.c_bb;
        double v = 0.0;
        if (lane == 0) v = cab;
        else if (lane == 1) v = caa;
        else if (lane == 2) v = cbb;
        else if (lane == 3) v = colour_tanimoto(cab, caa, cbb);
        else if (lane == 4) v = cbb == 0.0 ? 0.0 : cab / cbb;
        else if (lane == 5) v = caa == 0.0 ? 0.0 : cab / caa;
        else if (lane == 6) v = matched ? __builtin_sqrt(tA / (double)matched) : nan;
        a.summary[(size_t)row * 8 + lane] = ok ? v : nan;
    }
    if (lane < kT) {
        double v = 0.0;
#pragma unroll
        for (int k = 0; k < kT; ++k) v = lane == k ? ct[k] : v;
        a.type_overlap[(size_t)row * kT + lane] = ok ? v : nan;
    }
    if (lane < 4) {
        const int v = lane == 0 ? (int)nn : lane == 1 ? covered : lane == 2 ? ref_covered : (int)f;
        a.count[(size_t)row * 4 + lane] = ok ? v : 0;
    }
    if (lane < PMX_FINGERPRINT_WORDS) a.matched_fp[(size_t)row * PMX_FINGERPRINT_WORDS + lane] = lane == 0 ? fp : 0ull;
    if (lane == 0) a.status[row] = status;
}

void launch(const ColourArgs &a, hipStream_t stream) { colour_kernel<<<dim3((a.n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream>>>(a); }

// C_BB: the reference's own float32 features and masks as one feature-mode row under the identity motion, through the kernel every row takes.
hipError_t self_overlap(pmx_colour_ref *r, const float *xyz, const uint8_t *mask) {
    const uint32_t f = r->f;
    struct Fixed {
        double rot[9], trans[3], summary[8], type_overlap[kT], node_colour[kF], node_near[kF], feat_near[kF];
        uint64_t off[2], fp[PMX_FINGERPRINT_WORDS];
        float xyz[3 * kF];
        int32_t count[4], node_feature[kF], feat_node[kF], status[2];
        uint8_t mask[kF];
    };
    std::vector<Fixed> host(1);
    Fixed &fixed = host[0];
    fixed = Fixed{};
    fixed.rot[0] = fixed.rot[4] = fixed.rot[8] = 1.0;
    fixed.off[1] = f;
    for (uint32_t i = 0; i < f; ++i) {
        fixed.xyz[3 * i] = xyz[3 * i];
        fixed.xyz[3 * i + 1] = xyz[3 * i + 1];
        fixed.xyz[3 * i + 2] = xyz[3 * i + 2];
        fixed.mask[i] = mask[i];
    }
    Fixed *d = nullptr;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&d), sizeof(Fixed));
    if (e != hipSuccess) return e;
    e = hipMemcpy(d, &fixed, sizeof(Fixed), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        ColourArgs a{};
        a.ref = colour_ref_args(r);
        a.src.point_off = d->off;
        a.src.points = d->xyz;
        a.feat_mask = d->mask;
        a.rot = d->rot;
        a.trans = d->trans;
        a.n = 1;
        a.summary = d->summary;
        a.type_overlap = d->type_overlap;
        a.count = d->count;
        a.node_colour = d->node_colour;
        a.node_near = d->node_near;
        a.node_feature = d->node_feature;
        a.feat_near = d->feat_near;
        a.feat_node = d->feat_node;
        a.matched_fp = d->fp;
        a.status = d->status;
        launch(a, nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpy(&fixed, d, sizeof(Fixed), hipMemcpyDeviceToHost); // (waits for the kernel)
    }
    (void)hipFree(d);
    if (e == hipSuccess) r->c_bb = fixed.summary[1];
    return e;
}

// ---------------------------------------------------------------------------------------------------------------- pmx_combo_overlay
struct ComboArgs {
    const double4 *ref; // the shape reference
    uint32_t m;
    double o_bb;
    ColourRef colour;
    PoseSource src, node_src; // the shape points; the nodes (the same source where the shape points are the nodes)
    const double *rot, *trans;
    uint32_t n;
    float radius;
    double cw, ftol;
    int max_iter;
    double *rot_out, *trans_out, *energy;
    int32_t *count, *status;
};

struct ComboEval {
    double oab, cab;
    double c[3];
    double H[21], g[6];
};

// What pmx::lm_run follows: F = O_AB + cw * C_AB, up.
struct Combo {
    using Eval = ComboEval;
    const double4 *X; // the shape points, unposed, with their alphas
    uint32_t npts;
    const double4 *Lref;
    uint32_t m;
    double x0, x1, x2; // the lane's node, unposed
    uint32_t mk, nn;
    const double4 *Lfeat;
    const uint8_t *Lmask;
    ColourRef colour;
    double cw;
    int lane;

    __device__ __forceinline__ void eval(const double (&R)[9], const double (&t)[3], Eval &e) const {
        // ---- the colour pairs of the lane's node: cross, f and w need no centroid, so they are formed before the shape term and few values
        // live across it
        const bool mine = (uint32_t)lane < nn;
        double px = 0.0, py = 0.0, pz = 0.0;
        double cross = 0.0, f0 = 0.0, f1 = 0.0, f2 = 0.0, w = 0.0;
        if (mine) {
            pose_point(R, t, x0, x1, x2, px, py, pz);
            const double al = colour.alpha;
            const uint32_t f = colour.f;
#pragma unroll 1
            for (uint32_t b = 0; b < f; ++b) {
                const double pw = pair_weight(mk & (uint32_t)Lmask[b], colour);
                if (pw != 0.0) {
                    const double4 y = Lfeat[b];
                    const double e0 = px - y.x, e1 = py - y.y, e2 = pz - y.z;
                    const double d2 = (e0 * e0 + e1 * e1) + e2 * e2;
                    double k;
                    const double V = pw * pair_term(d2, al, al, k);
                    const double kappa = (2.0 * k) * V;
                    cross = cross + V;
                    f0 = f0 + kappa * e0;
                    f1 = f1 + kappa * e1;
                    f2 = f2 + kappa * e2;
                    w = w + kappa;
                }
            }
        }
        e.cab = scalar(wave_sum(cross));

        // ---- the shape term: O_AB, c, H_shape and g_shape
        ShapeEval s;
        pmx::shape_evaluate(X, npts, Lref, m, R, t, lane, s);
        e.oab = scalar(s.oab);
        e.c[0] = scalar(s.c[0]);
        e.c[1] = scalar(s.c[1]);
        e.c[2] = scalar(s.c[2]);

        // ---- the node's block, the shape term's with r = p - c, one value at a time (a lane has one node: its sum is 0.0 + the value);
        // H = H_shape + cw * H_colour and g likewise, value by value, after the butterfly
        const double r0 = px - s.c[0], r1 = py - s.c[1], r2 = pz - s.c[2];
        const double rr = (r0 * r0 + r1 * r1) + r2 * r2;
#define PMX_COLOUR_PART(expr) (cw * wave_sum(mine ? 0.0 + (expr) : 0.0))
#pragma unroll
        for (int k = 0; k < 21; ++k) e.H[k] = 0.0; // (H(0,3), H(1,4), H(2,5), H(3,4), H(3,5) and H(4,5) are 0 by structure)
        e.H[hidx(0, 0)] = scalar(s.H[hidx(0, 0)] + PMX_COLOUR_PART(w * (rr - r0 * r0)));
        e.H[hidx(0, 1)] = scalar(s.H[hidx(0, 1)] + PMX_COLOUR_PART(w * -(r0 * r1)));
        e.H[hidx(0, 2)] = scalar(s.H[hidx(0, 2)] + PMX_COLOUR_PART(w * -(r0 * r2)));
        e.H[hidx(1, 1)] = scalar(s.H[hidx(1, 1)] + PMX_COLOUR_PART(w * (rr - r1 * r1)));
        e.H[hidx(1, 2)] = scalar(s.H[hidx(1, 2)] + PMX_COLOUR_PART(w * -(r1 * r2)));
        e.H[hidx(2, 2)] = scalar(s.H[hidx(2, 2)] + PMX_COLOUR_PART(w * (rr - r2 * r2)));
        e.H[hidx(0, 4)] = scalar(s.H[hidx(0, 4)] + PMX_COLOUR_PART(w * -r2));
        e.H[hidx(0, 5)] = scalar(s.H[hidx(0, 5)] + PMX_COLOUR_PART(w * r1));
        e.H[hidx(1, 3)] = scalar(s.H[hidx(1, 3)] + PMX_COLOUR_PART(w * r2));
        e.H[hidx(1, 5)] = scalar(s.H[hidx(1, 5)] + PMX_COLOUR_PART(w * -r0));
        e.H[hidx(2, 3)] = scalar(s.H[hidx(2, 3)] + PMX_COLOUR_PART(w * -r1));
        e.H[hidx(2, 4)] = scalar(s.H[hidx(2, 4)] + PMX_COLOUR_PART(w * r0));
        e.H[hidx(3, 3)] = e.H[hidx(4, 4)] = e.H[hidx(5, 5)] = scalar(s.H[hidx(3, 3)] + PMX_COLOUR_PART(w));
        e.g[0] = scalar(s.g[0] + PMX_COLOUR_PART(r1 * f2 - r2 * f1));
        e.g[1] = scalar(s.g[1] + PMX_COLOUR_PART(r2 * f0 - r0 * f2));
        e.g[2] = scalar(s.g[2] + PMX_COLOUR_PART(r0 * f1 - r1 * f0));
        e.g[3] = scalar(s.g[3] + PMX_COLOUR_PART(f0));
        e.g[4] = scalar(s.g[4] + PMX_COLOUR_PART(f1));
        e.g[5] = scalar(s.g[5] + PMX_COLOUR_PART(f2));
#undef PMX_COLOUR_PART
    }
    __device__ __forceinline__ double value(const Eval &e) const { return e.oab + cw * e.cab; }
    __device__ __forceinline__ bool better(double trial, double cur) const { return trial > cur; }
    __device__ __forceinline__ double gain(double before, double after) const { return after - before; }
};

__global__ __launch_bounds__(64 * kWaves, 2) void combo_kernel(const ComboArgs a) {
    __shared__ double4 Lref[kA];
    __shared__ double4 Lx[kWaves][kA];
    __shared__ double4 Lp[kWaves][kA];
    __shared__ double4 Lfeat[kF];
    __shared__ uint8_t Lmask[kF];
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x / 64));
    const uint32_t row = blockIdx.x * kWaves + (uint32_t)wave;
    const bool live = row < a.n;
    const int lane = (int)(threadIdx.x % 64);

    pmx::stage_reference(Lref, a.ref, a.m);
    stage_features(a.colour, Lfeat, Lmask);

    // ---- the row's shape points - unposed with their alphas, and posed at the input motion - and the lane's node
    double R0[9], t0[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R0[k] = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) t0[k] = 0.0;
    int status = PMX_LIGAND_OK;
    uint32_t npts = 0, nn = 0, mk = 0;
    double x0 = 0.0, x1 = 0.0, x2 = 0.0;
    double4 *X = Lx[wave], *P = Lp[wave];
    if (live) {
        const bool finite = pose_motion(a.rot, a.trans, row, R0, t0);
        const PoseRow nr = pose_row(a.node_src, row, finite);
        const PoseRow pr = pose_row(a.src, row, finite);
        status = nr.status != PMX_LIGAND_OK ? nr.status : pr.status;
        npts = pr.npts;
        nn = nr.npts;
        if (status == PMX_LIGAND_OK && npts > (uint32_t)kA) status = PMX_LIGAND_UNSUPPORTED; // (more points than a molecule of the atom store can have)
        if (status != PMX_LIGAND_OK) npts = nn = 0;
        bool bad = pmx::stage_points<true>(pr, npts, R0, t0, a.radius, lane, P, X);
        if (nn) {
            const uint8_t *masks = record_masks(a.node_src, row);
            if ((uint32_t)lane < nn) {
                pose_load(nr, (uint32_t)lane, x0, x1, x2);
                mk = masks[lane];
                bad = bad || mk >= 128u;
            }
        }
        if (__ballot(bad) != 0ull) { // (a radius that is none, a mask of more than 7 bits: one ballot)
            status = PMX_LIGAND_KEY_INVALID;
            npts = nn = mk = 0;
        }
    }
    __syncthreads();
    if (!live) return;

    if (status != PMX_LIGAND_OK) {
        store_not_ok<16, 6>(a.rot_out, a.trans_out, a.energy, a.count, a.status, row, lane, status);
        return;
    }
    const uint32_t m = a.m;

    // ---- O_AA and C_AA, once, of the points and the nodes posed at the input motion: pmx_pose_shape's and pmx_pose_colour's terms
    const double oaa = scalar(wave_sum(pmx::self_overlap(P, npts, lane)));
    double caa;
    {
        double p0 = 0.0, p1 = 0.0, p2 = 0.0;
        if ((uint32_t)lane < nn) pose_point(R0, t0, x0, x1, x2, p0, p1, p2);
        caa = scalar(wave_sum(colour_self(p0, p1, p2, mk, nn, lane, a.colour)));
    }

    // ---- the iteration, from the evaluation at the start. F not > 0 - no point and no typed pair, or a row so far away that every term
    // underflows: nothing to follow
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k] = R0[k];
#pragma unroll
    for (int k = 0; k < 3; ++k) t[k] = t0[k];
    const Combo obj{X, npts, Lref, m, x0, x1, x2, mk, nn, Lfeat, Lmask, a.colour, a.cw, lane};
    ComboEval cur;
    obj.eval(R, t, cur);
    const double o_start = cur.oab, c_start_ab = cur.cab;
    const double c_start[3] = {cur.c[0], cur.c[1], cur.c[2]};
    const LmRun run = lm_run(obj, cur, R, t, obj.value(cur) > 0.0, a.ftol, a.max_iter);
    const double O = cur.oab, C = cur.cab; // (the last accepted evaluation's)

    // ---- the row's outputs: the last accepted motion (the input's own bits when nothing was accepted)
    double angle, shift;
    lm_net_motion(R, R0, run.accepted, cur.c, c_start, angle, shift);
    store_motion(a.rot_out, a.trans_out, row, lane, R, t);
    const double obb = a.o_bb, cbb = a.colour.c_bb;
    const double ts0 = tanimoto(o_start, oaa, obb), ts1 = tanimoto(O, oaa, obb), tc0 = colour_tanimoto(c_start_ab, caa, cbb), tc1 = colour_tanimoto(C, caa, cbb);
    const double en[16] = {o_start, O, oaa, obb, ts0, ts1, c_start_ab, C, caa, cbb, tc0, tc1, ts0 + tc0, ts1 + tc1, angle, shift};
    double out = 0.0;
#pragma unroll
    for (int k = 0; k < 16; ++k) out = lane == k ? en[k] : out;
    if (lane < 16) a.energy[(size_t)row * 16 + lane] = out;
    if (lane < 6) {
        const int v = lane == 0 ? run.iterations : lane == 1 ? run.accepted : lane == 2 ? run.reason : lane == 3 ? (int)npts : lane == 4 ? (int)nn : (int)a.colour.f;
        a.count[(size_t)row * 6 + lane] = v;
    }
    if (lane == 0) a.status[row] = status;
}

} // namespace

extern "C" int pmx_colour_ref_create(const float *xyz, const uint8_t *typemask, uint32_t f, const float weights[PMX_NUM_TYPES], float radius, int device, pmx_colour_ref **out) {
    if (!out) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: null out");
    *out = nullptr;
    if (f < 1 || f > (uint32_t)kF) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: %u features, 1 to %d", f, kF);
    if (!xyz || !typemask || !weights) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: null xyz, typemask or weights");
    if (!radius_ok(radius)) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: the radius is not a finite number > 0");
    for (int t = 0; t < kT; ++t)
        if (!std::isfinite(weights[t]) || !(weights[t] >= 0.0f)) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: weight %d is negative or not finite", t);
    std::vector<double4> feat(f);
    for (uint32_t i = 0; i < f; ++i) {
        if (!std::isfinite(xyz[3 * i]) || !std::isfinite(xyz[3 * i + 1]) || !std::isfinite(xyz[3 * i + 2]))
            return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: feature %u has a coordinate that is not finite", i);
        if (typemask[i] >= 128) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_create: feature %u has type mask %u, at most 127", i, (unsigned)typemask[i]);
        feat[i] = make_double4((double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2], 0.0);
    }
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_colour_ref_create: hipSetDevice failed");
    pmx_colour_ref *r = new pmx_colour_ref;
    r->device = device;
    r->f = f;
    r->alpha = pmx::alpha_of(radius);
    for (int t = 0; t < kT; ++t) r->w[t] = (double)weights[t];
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&r->feat), sizeof(double4) * f + f);
    if (e == hipSuccess) {
        r->mask = reinterpret_cast<uint8_t *>(r->feat + f);
        e = hipMemcpy(r->feat, feat.data(), sizeof(double4) * f, hipMemcpyHostToDevice);
    }
    if (e == hipSuccess) e = hipMemcpy(r->mask, typemask, f, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = self_overlap(r, xyz, typemask);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (r->feat) (void)hipFree(r->feat);
        delete r;
        return pmx_fail(e == hipErrorOutOfMemory ? PMX_ERR_OOM : PMX_ERR_HIP, "pmx_colour_ref_create: %s", hipGetErrorString(e));
    }
    *out = r;
    return PMX_OK;
}

extern "C" int pmx_colour_ref_self(const pmx_colour_ref *ref, double *self_out) {
    if (!ref || !self_out) return pmx_fail(PMX_ERR_INVALID, "pmx_colour_ref_self: null argument");
    *self_out = ref->c_bb;
    return PMX_OK;
}

extern "C" int pmx_colour_ref_destroy(pmx_colour_ref *ref) {
    if (!ref) return PMX_OK;
    if (ref->feat) {
        if (hipSetDevice(ref->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_colour_ref_destroy: hipSetDevice failed");
        (void)hipFree(ref->feat);
    }
    delete ref;
    return PMX_OK;
}

extern "C" int pmx_pose_colour(const pmx_colour_ref *ref, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev, const uint64_t *feat_off_dev,
                               const float *feat_xyz_dev, const uint8_t *feat_mask_dev, const double *rot_dev, const double *trans_dev, uint32_t n, float cover,
                               double *summary_dev, double *type_overlap_dev, int32_t *count_dev, double *node_colour_dev, double *node_near_dev, int32_t *node_feature_dev,
                               double *feat_near_dev, int32_t *feat_node_dev, uint64_t *matched_fp_dev, int32_t *status_dev, void *stream_) {
    if (!ref) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_colour: null reference");
    ColourArgs a{};
    if (lib && feat_mask_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_colour: a library and points: one source of points per call");
    const int rc = pmx::pose_source("pmx_pose_colour", "reference", ref->device, lib, ligands_dev, conformer_dev, feat_off_dev, feat_xyz_dev, nullptr, rot_dev, trans_dev, n, &a.src);
    if (rc != PMX_OK) return rc;
    if (!std::isfinite(cover) || cover < 0.0f) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_colour: cover must be finite and >= 0");
    if (n == 0) return PMX_OK;
    if (!lib && !feat_mask_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_pose_colour: null feat_mask_dev");
    if (!summary_dev || !type_overlap_dev || !count_dev || !node_colour_dev || !node_near_dev || !node_feature_dev || !feat_near_dev || !feat_node_dev || !matched_fp_dev || !status_dev)
        return pmx_fail(PMX_ERR_INVALID, "pmx_pose_colour: null output");
    if (hipSetDevice(ref->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_pose_colour: hipSetDevice failed");
    a.ref = colour_ref_args(ref);
    a.feat_mask = feat_mask_dev;
    a.rot = rot_dev;
    a.trans = trans_dev;
    a.n = n;
    a.cover = cover;
    a.summary = summary_dev;
    a.type_overlap = type_overlap_dev;
    a.count = count_dev;
    a.node_colour = node_colour_dev;
    a.node_near = node_near_dev;
    a.node_feature = node_feature_dev;
    a.feat_near = feat_near_dev;
    a.feat_node = feat_node_dev;
    a.matched_fp = matched_fp_dev;
    a.status = status_dev;
    launch(a, static_cast<hipStream_t>(stream_));
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_combo_overlay(const pmx_shape_ref *shape, const pmx_colour_ref *colour, const pmx_library *lib, const uint64_t *ligands_dev, const int32_t *conformer_dev,
                                 const uint64_t *point_off_dev, const float *points_dev, const float *point_radius_dev, const double *rot_dev, const double *trans_dev, uint32_t n,
                                 float point_radius, double colour_weight, double ftol, int max_iter, double *rot_out_dev, double *trans_out_dev, double *energy_dev,
                                 int32_t *count_dev, int32_t *status_dev, void *stream_) {
    if (!shape || !colour) return pmx_fail(PMX_ERR_INVALID, "pmx_combo_overlay: null %s reference", shape ? "colour" : "shape");
    if (shape->device != colour->device) return pmx_fail(PMX_ERR_INVALID, "pmx_combo_overlay: the shape reference is on device %d, the colour reference on %d", shape->device, colour->device);
    if (!lib) return pmx_fail(PMX_ERR_INVALID, "pmx_combo_overlay: null library: the colour points are the records' nodes");
    ComboArgs a{};
    const int rc = pmx::pose_source("pmx_combo_overlay", "reference", shape->device, lib, ligands_dev, conformer_dev, point_off_dev, points_dev, point_radius_dev, rot_dev, trans_dev, n,
                                    &a.src, true);
    if (rc != PMX_OK) return rc;
    if (!std::isfinite(point_radius)) return pmx_fail(PMX_ERR_INVALID, "pmx_combo_overlay: point_radius must be finite");
    if (const int bad = pmx::lm_check("pmx_combo_overlay", "ftol and colour_weight", ftol, max_iter, colour_weight)) return bad;
    if (n == 0) return PMX_OK;
    if (!rot_out_dev || !trans_out_dev || !energy_dev || !count_dev || !status_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_combo_overlay: null output");
    if (hipSetDevice(shape->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_combo_overlay: hipSetDevice failed");
    a.node_src = a.src;
    a.node_src.point_off = nullptr;
    a.node_src.points = nullptr;
    a.node_src.point_radius = nullptr;
    a.ref = shape->atoms;
    a.m = shape->m;
    a.o_bb = shape->o_bb;
    a.colour = colour_ref_args(colour);
    a.rot = rot_dev;
    a.trans = trans_dev;
    a.n = n;
    a.radius = point_radius;
    a.cw = colour_weight;
    a.ftol = ftol;
    a.max_iter = max_iter;
    a.rot_out = rot_out_dev;
    a.trans_out = trans_out_dev;
    a.energy = energy_dev;
    a.count = count_dev;
    a.status = status_dev;
    combo_kernel<<<dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, static_cast<hipStream_t>(stream_)>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
