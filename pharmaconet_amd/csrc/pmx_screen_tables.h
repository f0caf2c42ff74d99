// pmx_screen_tables.h - the table phase of the screening path (device): from a packed ligand record to its score tables and search
// bounds in a wave's slice or in the arena. The wave helpers, the pair-function builder (fn_build_kernel), the table items, scan_ligand,
// build_tables, chain_lengths, build_bounds and prepare_ligand, which strings them together. The product walker (pmx_screen_walk.h)
// and the explain walker (pmx_explain.hip) both start from what prepare_ligand leaves; the row kernels (pmx_rows.hip) take parse_record and the
// level rule (cluster_candidates, level_slot) only. Layouts: pmx_screen_layout.h (shared, namespace pmx) and pmx_screen_lds.h (per PMX_NS).
#pragma once
#include <type_traits>

#include "pmx_screen_lds.h"

// ---- tuning constants of this file (-D through PMX_CXXFLAGS or tools/build_variant.py; none changes a layout)
#ifndef PMX_ITEM_BATCH
#define PMX_ITEM_BATCH 2 // items whose loads are in flight together ([MI355X] 3: 108.5 against 106.7 ms per pass; 4 costs 30 spilled registers at 80)
#endif
#ifndef PMX_SELF_STAGE_MIN
#define PMX_SELF_STAGE_MIN 4 // (a cluster of two or three nodes has one or three self items: a staging trip - 16 node pairs wide, a round trip through LDS - costs more instructions than computing them in place)
#endif

// ---- instrumentation (analysis builds only; all off in the product, none changes a layout). What they count lands in WaveStats::dbg,
// which flush_wave_stats() adds to Ctl::stats[16 .. 21] and pmx_score_stats::dbg reports (tools/knob_sweep.py, tools/pocket_phases.py).
//   -DPMX_COUNTERS=1 | 2   walk(): 1 the kinds of passes, 2 what the bound test does (see the `dbg` array there)
//   -DPMX_TABLE_TICKS      s_memtime ticks of the parts of the table phase: [0] self tables [1] centres of a level pair [2] its node
//                          distances [3] prefilter and the rows of failing entries [4] items [5] chain lengths (build_bounds)
//   -DPMX_WALK_TICKS       s_memtime ticks inside path_bound() [0] and probe() [1]
//   -DPMX_TABLE_FILL       [1] wave-iterations of the pair items, [5] slot-items of them that belong to an entry
//   -DPMX_INJECT_VALU_ITEM=n, -DPMX_INJECT_VALU_WALK=n, -DPMX_INJECT_SALU_WALK=n
//                          n extra instructions of one kind per table item batch / per trip of the walker's loop: the slope of the pass
//                          time against n says which issue port a phase is bound by
//   -DPMX_CUT=bits         (with PMX_TREE_FLAGS=16384, tools/sq_cut.sh) 1 no self items, 2 no bounds pass, 4 no pair items - the instruction
//                          budget of a section is what its absence takes out of SQ_INSTS_*; scores are meaningless
#ifndef PMX_INJECT_VALU_ITEM
#define PMX_INJECT_VALU_ITEM 0
#endif
#ifndef PMX_INJECT_VALU_WALK
#define PMX_INJECT_VALU_WALK 0
#endif
#ifndef PMX_INJECT_SALU_WALK
#define PMX_INJECT_SALU_WALK 0
#endif
#ifndef PMX_CUT
#define PMX_CUT 0
#endif
// PMX_COUNT(i, n): counter i of walk()'s `dbg` array += n. PMX_TICK(i): the ticks since the last PMX_TICK of the function (its `tick_`) to
// WaveStats::dbg[i]; wants `lane`, `lds` and `ws` in scope.
#ifdef PMX_COUNTERS
#define PMX_COUNT(i, n) do { if (PMX_COUNTERS == 1 && (i) < 6) dbg[i] += (uint32_t)(n); } while (0)
#else
#define PMX_COUNT(i, n)
#endif
#ifdef PMX_TABLE_TICKS
#define PMX_TICK(i) do { const unsigned long long t_ = __builtin_amdgcn_s_memtime(); if (lane == 0) reinterpret_cast<WaveStats *>(lds + ws.off_stat)->dbg[i] += t_ - tick_; tick_ = t_; } while (0)
#else
#define PMX_TICK(i)
#endif

namespace PMX_NS {
using namespace pmx; // (pmx_device.h, pmx_screen_layout.h)

struct WaveStats { // lives in LDS (WaveShape::off_stat), updated by lane 0
    unsigned long long frames, passes, over, items, exact, longest, tasks, overflow;
    unsigned long long cyc_scan, cyc_tables, cyc_bounds, cyc_walk, exactv, npath, pad[2]; // s_memtime ticks per phase | self items evaluated term by term
    unsigned long long dbg[8]; // instrumented builds: see the list above
    unsigned long long dead, pad3; // pair entries the dead-entry test of build_tables settled without computing them
};
static_assert(sizeof(WaveStats) == 208, "WaveStats layout");

// ------------------------------------------------------------------------------------------------ helpers
// Instruction injection (PMX_INJECT_*, above)
template <int N>
__device__ __forceinline__ void inject_valu() {
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("v_nop");
}
template <int N>
__device__ __forceinline__ void inject_salu() {
    int x = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) asm volatile("s_add_u32 %0, %0, 1" : "+s"(x) : : "scc");
}

// A ligand's score: the float32 of the float64 mean the reference returns (graph_match.py:109), or that float64 itself (pmx_score_f64).
__device__ __forceinline__ void put_score(const ScreenParams &p, uint32_t li, double v) {
    // ([MI355X] A/B: the kernels always writing the float64 and a conversion kernel per chunk for pmx_score: 99.8 ms against 98.7-98.9 for this branch)
    if (p.flags & PMX_SCORES_F64) reinterpret_cast<double *>(p.scores)[li] = v;
    else p.scores[li] = (float)v;
}

__device__ inline int rl(int v, int lane) { return __builtin_amdgcn_readlane(v, lane); }
// lane `lane` (wave-uniform) of v := value (this clang has no v_writelane builtin; a compare + select does it)
__device__ inline int wl(int v, int lane, int value) { return (int)(threadIdx.x & 63) == lane ? value : v; }
// The lane id as a value the optimiser cannot see through: address arithmetic derived from it stays inside the loop that uses it
// (hoisted out of the persistent loops it was kept live - spilled - for the whole kernel).
__device__ inline int lane_id() {
    int l = (int)(threadIdx.x & 63);
    asm volatile("" : "+v"(l));
    return l;
}
__device__ inline int uni(int v) { return __builtin_amdgcn_readfirstlane(v); }
__device__ inline uint64_t uni64(uint64_t v) {
    return ((uint64_t)(uint32_t)uni((int)(v >> 32)) << 32) | (uint64_t)(uint32_t)uni((int)(uint32_t)v);
}
template <typename T>
__device__ inline T *uniptr(T *p) {
    return reinterpret_cast<T *>(uni64(reinterpret_cast<uint64_t>(p)));
}
// Largest value of the wavefront, in every lane: butterfly inside the rows of 16 lanes (DPP), then the four rows.
__device__ inline float wave_max_f32(float v) {
    int x = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0xB1, 0xf, 0xf, false))); // quad_perm [1,0,3,2]
    x = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x4E, 0xf, 0xf, false))); // quad_perm [2,3,0,1]
    x = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x124, 0xf, 0xf, false))); // row_ror:4
    x = __float_as_int(v);
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x128, 0xf, 0xf, false))); // row_ror:8
    x = __float_as_int(v);
    const float r0 = __int_as_float(__builtin_amdgcn_readlane(x, 0)), r1 = __int_as_float(__builtin_amdgcn_readlane(x, 16));
    const float r2 = __int_as_float(__builtin_amdgcn_readlane(x, 32)), r3 = __int_as_float(__builtin_amdgcn_readlane(x, 48));
    return fmaxf(fmaxf(r0, r1), fmaxf(r2, r3));
}
// Largest value over the lanes that stand for the same conformer (lane % G) in all 64 / G slots, in every lane: rotations
// inside the rows of 16 lanes (DPP), then the rows by the lane swaps of gfx950 (v_permlane16_swap / v_permlane32_swap) -
// no trip through the LDS crossbar (ds_bpermute, what __shfl_xor compiles to).
template <int G>
__device__ __forceinline__ float slot_max_f32(float v) {
    if (G <= 1) { const int x = __float_as_int(v); v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x121, 0xf, 0xf, false))); } // row_ror:1
    if (G <= 2) { const int x = __float_as_int(v); v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x122, 0xf, 0xf, false))); } // row_ror:2
    if (G <= 4) { const int x = __float_as_int(v); v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x124, 0xf, 0xf, false))); } // row_ror:4
    if (G <= 8) { const int x = __float_as_int(v); v = fmaxf(v, __int_as_float(__builtin_amdgcn_update_dpp(x, x, 0x128, 0xf, 0xf, false))); } // row_ror:8
    if (G <= 16) {
        const unsigned x = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane16_swap(x, x, false, false); // {rows 0 0 2 2, rows 1 1 3 3}
        v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    if (G <= 32) {
        const unsigned x = __float_as_uint(v);
        const auto r = __builtin_amdgcn_permlane32_swap(x, x, false, false); // {lower half twice, upper half twice}
        v = fmaxf(__uint_as_float(r[0]), __uint_as_float(r[1]));
    }
    return v;
}
__device__ inline void wave_sync() { // LDS / global hand-over between the lanes of one wavefront
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
}
// Hand-over through LDS only (does not wait for outstanding global stores)
__device__ inline void lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }
// The smallest float32 that is not below x (NaN stays NaN).
__device__ inline float float_up(double x) {
    const float f = (float)x;
    if (!((double)f < x)) return f;
    const uint32_t b = __float_as_uint(f);
    return __uint_as_float(f > 0.f ? b + 1u : (f < 0.f ? b - 1u : 1u));
}
// The smallest bfloat16 that is not below f, as its 16 bits (NaN stays NaN; +inf beyond the largest finite one - an upper bound either way).
__device__ inline uint16_t bf16_up(float f) {
    const uint32_t b = __float_as_uint(f);
    if (f != f) return (uint16_t)0x7fc0u;
    const uint32_t hi = b >> 16;
    if ((b & 0xffffu) == 0u || (b >> 31)) return (uint16_t)hi; // exact, or negative: dropping low bits moves a negative value up
    return (uint16_t)(hi + 1u);
}
__device__ inline float bf16_value(uint16_t h) { return __uint_as_float((uint32_t)h << 16); }
__device__ inline float norm3f(float dx, float dy, float dz) { // np.linalg.norm of a float32 3-vector (ligand.py:349-351)
    float s = dx * dx;
    s = s + dy * dy;
    s = s + dz * dz;
    return sqrtf(s);
}

// ------------------------------------------------------------------------------------ fn_build_kernel
// Tabulates F_(sa, sb)(d) for every pair of node subsets on the grid x_i = i * h: quintic Hermite cells from F, F', F''
// at the two ends of a cell, evaluated in float64. `win` holds the exact pass windows of every cell (host, model-only).
// A subset pair with a zero weight sum scores NaN in the reference (0 * (1 / 0), match_utils.py:50-52,69): NaN cells.
__global__ void fn_build_kernel(DevModel M, Weights W, const uint32_t *sub_off, const uint8_t *sub_nodes, uint32_t NS, uint32_t ncell, float h,
                                const float2 *win, FnCell *cells, double rel_tol, double max_exponent) {
    const uint32_t fid = blockIdx.x;
    uint32_t sa, sb;
    if (M.symmetric) { // triangular: fid = sa (sa + 1) / 2 + sb, sb <= sa
        sa = (uint32_t)((sqrtf(8.f * (float)fid + 1.f) - 1.f) * 0.5f);
        while ((sa + 1) * (sa + 2) / 2 <= fid) ++sa;
        while (sa * (sa + 1) / 2 > fid) --sa;
        sb = fid - sa * (sa + 1) / 2;
    } else {
        sa = fid / NS, sb = fid - sa * NS;
    }
    const uint8_t *A = sub_nodes + sub_off[sa], *B = sub_nodes + sub_off[sb];
    const int nA = (int)(sub_off[sa + 1] - sub_off[sa]), nB = (int)(sub_off[sb + 1] - sub_off[sb]);
    const int Nm = M.Nm;
    bool a_nz = false, b_nz = false;
    for (int i = 0; i < nA; ++i) a_nz = a_nz || W.w[M.node_type[A[i]]] != 0.f;
    for (int i = 0; i < nB; ++i) b_nz = b_nz || W.w[M.node_type[B[i]]] != 0.f;
    const bool empty = nA == 0 || nB == 0;
    const bool nanfn = !empty && (!a_nz || !b_nz);
    const double inv_mn = empty ? 0.0 : 1.0 / (double)(nA * nB);
    for (uint32_t i = threadIdx.x; i < ncell; i += blockDim.x) {
        double f[2], d1[2], d2[2];
        for (int e = 0; e < 2; ++e) {
            const double x = (double)(i + e) * (double)h;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0;
            if (!empty && !nanfn) {
                for (int ia = 0; ia < nA; ++ia) {
                    const int m = A[ia];
                    for (int ib = 0; ib < nB; ++ib) {
                        const int n = B[ib];
                        const float4 eg = M.edge[m * Nm + n]; // {mean, s, T, std}
                        const float wprod = W.w[M.node_type[m]] * W.w[M.node_type[n]];
                        const double coef = (double)(wprod / eg.w); // weights / stds in float32 (match_utils.py:65)
                        const double sd = (double)eg.w, z = (x - (double)eg.x) / sd;
                        const double g = exp(-0.5 * z * z);
                        s0 += coef * g;
                        s1 += coef * g * (-z / sd);
                        s2 += coef * g * ((z * z - 1.0) / (sd * sd));
                    }
                }
            }
            f[e] = s0 * inv_mn;
            d1[e] = s1 * inv_mn * (double)h;
            d2[e] = s2 * inv_mn * (double)h * (double)h;
        }
        const double df = f[1] - f[0];
        FnCell c;
        c.c[0] = (float)f[0];
        c.c[1] = (float)d1[0];
        c.c[2] = (float)(0.5 * d2[0]);
        c.c[3] = (float)(10.0 * df - 6.0 * d1[0] - 4.0 * d1[1] - 1.5 * d2[0] + 0.5 * d2[1]);
        c.c[4] = (float)(-15.0 * df + 8.0 * d1[0] + 7.0 * d1[1] + 1.5 * d2[0] - d2[1]);
        c.c[5] = (float)(6.0 * df - 3.0 * d1[0] - 3.0 * d1[1] - 0.5 * d2[0] + 0.5 * d2[1]);
        // worst deviation of the float32 polynomial from the function, relative to the function, at eight points inside the cell
        bool rough = i + 1 == ncell; // (the last cell is also where every distance beyond the grid lands)
        if (!empty && !nanfn && !rough) {
            for (int k = 0; k < 8 && !rough; ++k) {
                const double t = ((double)k + 0.5) * 0.125, x = ((double)i + t) * (double)h;
                double s0 = 0.0, e0 = 0.0;
                for (int ia = 0; ia < nA; ++ia) {
                    const int m = A[ia];
                    for (int ib = 0; ib < nB; ++ib) {
                        const int n = B[ib];
                        const float4 eg = M.edge[m * Nm + n];
                        const float wprod = W.w[M.node_type[m]] * W.w[M.node_type[n]];
                        const double z = (x - (double)eg.x) / (double)eg.w;
                        const double g = (double)(wprod / eg.w) * exp(-0.5 * z * z);
                        s0 += g;
                        e0 += g * (0.5 * z * z);
                    }
                }
                const double fx = s0 * inv_mn;
                const double px = (double)c.c[0] + t * ((double)c.c[1] + t * ((double)c.c[2] + t * ((double)c.c[3] + t * ((double)c.c[4] + t * (double)c.c[5]))));
                // ... and where the function is down to exp(-max_exponent) of its terms' peaks: the reference computes z and z^2 in
                // float32, which moves exp(-z^2 / 2) by up to 1.8e-7 z^2 / 2 of its value - rounding a smooth table cannot follow
                rough = fabs(px - fx) > rel_tol * fx || e0 > max_exponent * s0;
            }
        }
        c.c[5] = __uint_as_float((__float_as_uint(c.c[5]) & ~1u) | (rough ? 1u : 0u));
        if (nanfn) c.c[0] = __builtin_nanf("");
        const float2 w = win[(size_t)fid * ncell + i];
        c.lo = w.x;
        c.hi = w.y;
        float4 *planes = reinterpret_cast<float4 *>(cells);
        planes[(size_t)fid * ncell + i] = make_float4(c.c[0], c.c[1], c.c[2], c.c[3]);
        planes[(size_t)gridDim.x * ncell + (size_t)fid * ncell + i] = make_float4(c.c[4], c.c[5], c.lo, c.hi);
    }
}

// the conformers of one slot, as bits
template <int G>
__host__ __device__ constexpr uint64_t group_mask() {
    return G >= 64 ? ~0ull : ((1ull << (G & 63)) - 1ull);
}
constexpr double kBoundSlack = 1.0 + 1e-9; // on every bound test of the walkers: covers the float64 rounding of the sums the bound is compared with

// ------------------------------------------------------------------------------------------ table phase
// Round 6: instruction injection (inject_valu / inject_salu above) showed that every instruction of a table item costs its full issue price -
// 16 / 32 v_nops per batch of two items: tables alone 43.5 -> 45.3 / 47.7 ms - so the item is on a diet: the function index of a symmetric model
// (every model the reference can make) without the general form and its 64-bit multiply-add, the cell number kept as the integer it is, 24-bit
// multiplies where an entry is decoded.
// TRI: the caller has established that the table is triangular (FnTable::tri, wave-uniform)
template <bool TRI>
__device__ __forceinline__ uint32_t fn_index_t(const FnTable &F, uint32_t sidu, uint32_t sidv) {
    if (TRI) {
        const uint32_t hi = max(sidu, sidv), lo = min(sidu, sidv);
        return ((__umul24(hi, hi) + hi) >> 1) + lo; // (subset ids are 16 bits)
    }
    return __umul24(sidu, F.NS) + sidv;
}
__device__ __forceinline__ uint32_t fn_index(const FnTable &F, uint32_t sidu, uint32_t sidv) {
    // (both forms and a bit select on the wave-uniform `tri`: a branch here is a branch per table item)
    const uint32_t hi = max(sidu, sidv), lo = min(sidu, sidv);
    const uint32_t t = (__umul24(hi, hi + 1u) >> 1) + lo, f = __umul24(sidu, F.NS) + sidv; // (subset ids are 16 bits)
    const uint32_t m = 0u - F.tri;
    return (t & m) | (f & ~m);
}

// One (ligand node, ligand node) item term by term, in the float32 operations of the reference (match_utils.py:50-69 and
// :108-120; same order as oracle/pmx_oracle.c node_pair_term): weights_sum by float32 additions, z = (d - mean) / std with
// an IEEE division, exp(-0.5 z^2) to float32 accuracy, the likelihood added up in the order of itertools.product, then
// likelihood * (1 / weights_sum) * (weights_sum / num_match). A subset pair whose weights sum to 0 gives NaN like the
// reference (x * inf * 0). np = the terms within 2 sigma (:56-60). A, B non-empty.
__device__ __forceinline__ float exact_value(const ScreenParams &p, uint32_t sidu, uint32_t sidv, float d, int &np, int &mn) {
    const uint8_t *A = p.sub_nodes + p.sub_off[sidu], *B = p.sub_nodes + p.sub_off[sidv];
    const int nA = (int)(p.sub_off[sidu + 1] - p.sub_off[sidu]), nB = (int)(p.sub_off[sidv + 1] - p.sub_off[sidv]);
    float weights_sum = 0.f;
    for (int ia = 0; ia < nA; ++ia) {
        const float wa = p.W.w[p.M.node_type[A[ia]]];
        for (int ib = 0; ib < nB; ++ib) weights_sum = weights_sum + wa * p.W.w[p.M.node_type[B[ib]]];
    }
    mn = nA * nB;
    const float normalize_coeff = 1.0f / weights_sum, score_coeff = weights_sum / (float)mn;
    float likelihood = 0.f;
    np = 0;
    for (int ia = 0; ia < nA; ++ia) {
        const int m = A[ia];
        const float wa = p.W.w[p.M.node_type[m]];
        for (int ib = 0; ib < nB; ++ib) {
            const int n = B[ib];
            const float4 e = p.M.edge[m * p.M.Nm + n]; // {mean, s, T, std}
            const float t = d - e.x, z = t / e.w;
            np += fabsf(t) <= e.z ? 1 : 0; // == abs(z) < 2 (pmx_device.h)
            const float wos = (wa * p.W.w[p.M.node_type[n]]) / e.w;
            likelihood = likelihood + wos * expf(-0.5f * (z * z));
        }
    }
    return likelihood * normalize_coeff * score_coeff;
}
// The terms of the subset pair within 2 sigma at distance d against half of their number (match_utils.py:56-61): does the item fail?
__device__ __forceinline__ bool majority_fails(const ScreenParams &p, uint32_t sidu, uint32_t sidv, float d) {
    const uint8_t *A = p.sub_nodes + p.sub_off[sidu], *B = p.sub_nodes + p.sub_off[sidv];
    const int nA = (int)(p.sub_off[sidu + 1] - p.sub_off[sidu]), nB = (int)(p.sub_off[sidv + 1] - p.sub_off[sidv]);
    int np = 0;
    for (int ia = 0; ia < nA; ++ia)
        for (int ib = 0; ib < nB; ++ib) {
            const float4 e = p.M.edge[(int)A[ia] * p.M.Nm + (int)B[ib]];
            np += fabsf(d - e.x) <= e.z ? 1 : 0;
        }
    return 2 * np < nA * nB;
}

// One (ligand node, ligand node) item of match_utils.py:26-69 for the subset pair (sidu, sidv) at distance d: the tabulated
// sum (already divided by |A||B|) and whether the item fails the majority test of :56-61. SELF: the item belongs to a self
// entry, where a cell flagged as rough (FnCell) is evaluated term by term. EXACT (PMX_TREE_FLAGS & 8): every item is.
template <bool EXACT, bool SELF>
__device__ __forceinline__ void item(const ScreenParams &p, uint32_t sidu, uint32_t sidv, float d, float &acc, int &fails,
                                     uint32_t &n_exact, uint32_t &n_exactv) {
    if (!EXACT) {
        const float x = d * p.F.inv_h; // exact: inv_h is a power of two
        const int ci = min((int)x, (int)p.F.ncell - 1);
        const float t = fminf(x - (float)ci, 1.0f);
        const float4 *cell = reinterpret_cast<const float4 *>(p.F.cells) + (fn_index(p.F, sidu, sidv) * p.F.ncell + (uint32_t)ci);
        const float4 a = cell[0], b = cell[p.F.plane16];
        float v = __builtin_fmaf(t, b.y, b.x);
        v = __builtin_fmaf(t, v, a.w);
        v = __builtin_fmaf(t, v, a.z);
        v = __builtin_fmaf(t, v, a.y);
        v = __builtin_fmaf(t, v, a.x);
        if (SELF) {
            if (__builtin_expect((__float_as_uint(b.y) & 1u) != 0u && sidu != 0u && sidv != 0u, 0)) {
                int np, mn;
                v = exact_value(p, sidu, sidv, d, np, mn);
                ++n_exactv;
            }
            acc = acc + v;
            return; // (no majority test on self entries)
        }
        acc = acc + v;
        if (__builtin_expect(b.z != b.z, 0)) { // the pass set is not one interval inside this cell: count the terms
            fails += majority_fails(p, sidu, sidv, d) ? 1 : 0;
            ++n_exact;
        } else {
            fails += (d >= b.z && d <= b.w) ? 0 : 1;
        }
        return;
    }
    // debug / validation (flags & 8): every item term by term
    if (sidu == 0u || sidv == 0u) return; // (0 = the empty subset)
    int np, mn;
    acc = acc + exact_value(p, sidu, sidv, d, np, mn);
    fails += 2 * np < mn ? 1 : 0;
}

// The same item in two steps, so that the loads of several items are in flight together: address + loads, then value + test.
// (What an item holds while its cell is on the way is what limits how many can be: the cell, the distance, the two subset ids
// in one word; the position inside the cell is worked out again from the distance.)
struct ItemLoad {
    float4 a, b;
    float d, cell; // the distance and the number of its cell (as a float: the position inside the cell is d / h - cell)
    uint32_t sids; // sidu | sidv << 16
};
// the cell of a distance: min(floor(d / h), ncell - 1)
__device__ __forceinline__ float cell_of(const ScreenParams &p, float d) {
    return (float)min((int)(d * p.F.inv_h), (int)p.F.ncell - 1); // (d * inv_h is exact: inv_h is a power of two)
}
// (the diet's form: the function index by the caller's knowledge of the table's shape, the cell number computed once)
template <bool TRI>
__device__ __forceinline__ ItemLoad item_load_t(const ScreenParams &p, uint32_t sidu, uint32_t sidv, float d) {
    ItemLoad L;
    L.d = d;
    const int ci = min((int)(d * p.F.inv_h), (int)p.F.ncell - 1);
    L.cell = (float)ci;
    L.sids = sidu | (sidv << 16);
    const uint32_t off = (__umul24(fn_index_t<TRI>(p.F, sidu, sidv), p.F.ncell) + (uint32_t)ci) << 4;
    const unsigned char *pa = reinterpret_cast<const unsigned char *>(p.F.cells);
    const unsigned char *pb = pa + (size_t)p.F.plane16 * 16u;
    L.a = *reinterpret_cast<const float4 *>(pa + off);
    L.b = *reinterpret_cast<const float4 *>(pb + off);
    return L;
}
__device__ __forceinline__ ItemLoad item_load(const ScreenParams &p, uint32_t sidu, uint32_t sidv, float d, float cell) {
    ItemLoad L;
    L.d = d;
    L.cell = cell;
    L.sids = sidu | (sidv << 16);
    // (functions x cells < 2^27 - the table is addressed with 32 bits - and a function has hundreds of cells: 24-bit factors)
    const uint32_t off = (__umul24(fn_index(p.F, sidu, sidv), p.F.ncell) + (uint32_t)(int)cell) << 4;
    const unsigned char *pa = reinterpret_cast<const unsigned char *>(p.F.cells);
    const unsigned char *pb = pa + (size_t)p.F.plane16 * 16u; // (both planes: uniform base + 32-bit lane offset)
    L.a = *reinterpret_cast<const float4 *>(pa + off);
    L.b = *reinterpret_cast<const float4 *>(pb + off);
    return L;
}
// TAILS: the call's type weights differ by more than PMX_TAILS_RATIO (pmx_api.hip) - a pair item honours the rough-cell flag like a
// self item. With the reference's default weights (8 : 1 at most) an entry that counts is made of items near their functions' peaks, next
// to which the error of a tail value is below float32 rounding; with `--cation 100 --hydrophobic 0.1` (screening.py:54-62) an entry can
// be a handful of passing Hydrophobic items beside one failing Cation x Cation item five sigma out whose function is 10^6 times theirs -
// and the tail IS the entry (tests/test_gpu_pair_tails.py).
template <bool TAILS>
__device__ __forceinline__ void item_finish(const ScreenParams &p, const ItemLoad &L, float &acc, int &fails, uint32_t &n_exact, uint32_t &n_exactv) {
    if (TAILS) {
        const uint32_t su = L.sids & 0xffffu, sv = L.sids >> 16;
        if (__builtin_expect((__float_as_uint(L.b.y) & 1u) != 0u && su != 0u && sv != 0u, 0)) {
            int np, mn;
            acc = acc + exact_value(p, su, sv, L.d, np, mn);
            fails += 2 * np < mn ? 1 : 0; // match_utils.py:56-61
            ++n_exactv;
            return;
        }
    }
    const float t = fminf(__builtin_fmaf(L.d, p.F.inv_h, -L.cell), 1.0f); // (= d / h - cell exactly: the product is exact)
    float v = __builtin_fmaf(t, L.b.y, L.b.x);
    v = __builtin_fmaf(t, v, L.a.w);
    v = __builtin_fmaf(t, v, L.a.z);
    v = __builtin_fmaf(t, v, L.a.y);
    v = __builtin_fmaf(t, v, L.a.x);
    acc = acc + v;
    // lo <= d <= hi as "d is the median of (d, lo, hi)" (every window has lo <= hi; pmx_model_tables.cpp cell_windows): one compare, no mask arithmetic. A cell whose
    // pass set is not one interval (lo = NaN; 0.8 items per ligand) is put right behind one wave-wide test instead of an exec-mask detour per item.
    const bool fail = __builtin_amdgcn_fmed3f(L.d, L.b.z, L.b.w) != L.d;
    fails += fail ? 1 : 0;
    if (__builtin_expect(__ballot(L.b.z != L.b.z) != 0ull, 0)) {
        if (L.b.z != L.b.z) { // count the terms
            fails += (majority_fails(p, L.sids & 0xffffu, L.sids >> 16, L.d) ? 1 : 0) - (fail ? 1 : 0);
            ++n_exact;
        }
    }
}

struct LevelInfo {
    int nl;
    uint32_t ksumtot, T;
};

// Cluster candidates and tree levels (graph_match.py:124-137, :87-88) of the record, into the wave's LDS: clusters arrive
// sorted by priority_fn; a cluster is kept if some model cluster shares a type with it; at most 20 are kept. Then the
// node-candidate table nc[level][candidate][node] = node subset of the model cluster compatible with the ligand node
// (graph_match.py:145-155) and the counts L of ligand nodes with a non-empty subset (graph_match.py:164-171).
template <int G>
__device__ __forceinline__ LevelInfo scan_ligand(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, const Record &r) {
    const int lane = lane_id();
    uint8_t *tm = lds + kOffTm, *lstart = lds + kOffStart, *lend = lds + kOffEnd, *lk = lds + kOffK;
    uint16_t *ksum = reinterpret_cast<uint16_t *>(lds + kOffKsum), *ncoff = reinterpret_cast<uint16_t *>(lds + kOffNcoff);
    uint32_t *rowbase = reinterpret_cast<uint32_t *>(lds + kOffRow);
    uint32_t *scal = reinterpret_cast<uint32_t *>(lds + kOffBits + 8 * PMX_MAX_LEVELS); // ksumtot, T
    uint8_t *cand = lds + ws.off_cand, *lcnt = lds + ws.off_lcnt;
    uint16_t *nc = reinterpret_cast<uint16_t *>(lds + ws.off_nc);
    if (lane < r.n) tm[lane] = r.typemask[lane];
    wave_sync();
    int cs = 0, ce = 0;
    uint64_t cb0 = 0, cb1 = 0; // candidate clusters of the ligand cluster (PMX_MAX_MODEL_CLUSTERS bits)
    if (lane < r.ncl) {
        cs = lane ? r.cluster_end[lane - 1] : 0;
        ce = r.cluster_end[lane];
        unsigned lm = 0;
        for (int u = cs; u < ce; ++u) lm |= tm[u];
        cb0 = p.M.tclus[2u * (lm & 127u)];
        cb1 = p.M.tclus[2u * (lm & 127u) + 1u];
    }
    const bool has = (cb0 | cb1) != 0ull;
    const int kc = (int)__popcll(cb0) + (int)__popcll(cb1);
    const unsigned long long bal = __ballot(has);
    const int lev = __popcll(bal & ((1ull << lane) - 1ull));
    const int nl = min((int)__popcll(bal), PMX_MAX_LEVELS);
    // (a level's candidates are a 64-bit set in the walker: a ligand cluster with more - only a model of more than 64 clusters has
    // that many of one type - makes the ligand unsupported)
    if (__ballot(has && lev < PMX_MAX_LEVELS && kc > PMX_MAX_LEVEL_CANDIDATES) != 0ull) {
        LevelInfo bad;
        bad.nl = -1, bad.ksumtot = 0, bad.T = 0;
        return bad;
    }
    if (has && lev < PMX_MAX_LEVELS) {
        lstart[lev] = (uint8_t)cs;
        lend[lev] = (uint8_t)ce;
        lk[lev] = (uint8_t)kc;
        int q = 0;
        for (uint64_t x = cb0; x; x &= x - 1, ++q) cand[lev * ws.kp + q] = (uint8_t)(__ffsll((unsigned long long)x) - 1);
        for (uint64_t x = cb1; x; x &= x - 1, ++q) cand[lev * ws.kp + q] = (uint8_t)(64 + __ffsll((unsigned long long)x) - 1);
    }
    wave_sync();
    if (lane == 0) {
        uint32_t ks = 0, no = 0;
        for (int l = 0; l < nl; ++l) {
            ksum[l] = (uint16_t)ks;
            ncoff[l] = (uint16_t)no;
            ks += lk[l];
            no += (uint32_t)lk[l] * (uint32_t)(lend[l] - lstart[l]);
        }
        ksum[nl] = (uint16_t)ks;
        uint32_t rb = 0, run = 0;
        for (int l = 0; l < nl; ++l) {
            rowbase[l] = rb;
            run += lk[l];
            rb += (uint32_t)lk[l] * (ks - run);
        }
        scal[0] = ks;
        scal[1] = rb;
    }
    wave_sync();
    for (int l = 0; l < nl; ++l) {
        const int s0 = uni(lstart[l]), n = uni(lend[l]) - s0, k = uni(lk[l]), base = uni(ncoff[l]);
        const float inv_n = 1.0f / (float)n;
        for (int idx = lane; idx < k * n; idx += 64) {
            const int q = (int)(((float)idx + 0.5f) * inv_n), u = idx - q * n;
            nc[base + idx] = p.sidtab[(uint32_t)cand[l * ws.kp + q] * 128u + tm[s0 + u]];
        }
    }
    wave_sync();
    for (int l = 0; l < nl; ++l) {
        const int n = uni(lend[l]) - uni(lstart[l]), k = uni(lk[l]), base = uni(ncoff[l]);
        if (lane < k) {
            int cnt = 0;
            for (int u = 0; u < n; ++u) cnt += nc[base + lane * n + u] != 0 ? 1 : 0;
            lcnt[l * ws.kp + lane] = (uint8_t)cnt;
        }
    }
    wave_sync();
    LevelInfo L;
    L.nl = nl;
    L.ksumtot = (uint32_t)uni((int)scal[0]);
    L.T = (uint32_t)uni((int)scal[1]);
    return L;
}

// The same level rule for the kernels that open one listed ligand outside the score pass (pmx_rows.hip, explain_walk): which tree a key
// talks about. scan_ligand keeps its own lines - the score pass is bound by instruction issue and tuned as it stands - so a change of the
// rule is made there and here.
// What lane `lane` knows about ligand cluster `lane` (< ncl) of the record: its nodes [cs, ce) and the model clusters that share a type
// with one of them (PMX_MAX_MODEL_CLUSTERS bits); zeros in the other lanes. tm(u): type mask of node u.
struct ClusterCand {
    int cs, ce;
    unsigned long long cb0, cb1;
};
template <class TypeMask>
__device__ __forceinline__ ClusterCand cluster_candidates(const ScreenParams &p, const Record &r, int ncl, int lane, TypeMask tm) {
    ClusterCand k{0, 0, 0ull, 0ull};
    if (lane < ncl) {
        k.cs = lane ? r.cluster_end[lane - 1] : 0;
        k.ce = r.cluster_end[lane];
        unsigned lm = 0;
        for (int u = k.cs; u < k.ce; ++u) lm |= tm(u);
        k.cb0 = p.M.tclus[2u * (lm & 127u)];
        k.cb1 = p.M.tclus[2u * (lm & 127u) + 1u];
    }
    return k;
}
// The ballot over the wavefront's clusters: `has` a candidate, then level `lev` of the tree when lev < nl (priority order, at most
// PMX_MAX_LEVELS); too_many: a level has more than PMX_MAX_LEVEL_CANDIDATES candidates, which makes the ligand unsupported.
struct LevelSlot {
    bool has;
    int lev, nl;
    bool too_many;
};
__device__ __forceinline__ LevelSlot level_slot(const ClusterCand &k, int lane) {
    LevelSlot s;
    s.has = (k.cb0 | k.cb1) != 0ull;
    const int kc = (int)__popcll(k.cb0) + (int)__popcll(k.cb1);
    const unsigned long long bal = __ballot(s.has);
    s.lev = __popcll(bal & ((1ull << lane) - 1ull));
    s.nl = min((int)__popcll(bal), PMX_MAX_LEVELS);
    s.too_many = __ballot(s.has && s.lev < PMX_MAX_LEVELS && kc > PMX_MAX_LEVEL_CANDIDATES) != 0ull;
    return s;
}

struct Pos3 {
    float x, y, z;
};

// LigandNodeCluster.center / .size for one conformer (ligand.py:458-473).
// (a pointer into device memory, said so: a generic pointer costs flat loads, which also wait on the LDS counter, and 64-bit
// address arithmetic per load)
typedef const __attribute__((address_space(1))) float *GlobalFloats;
__device__ __forceinline__ void center_size(GlobalFloats xyz, int C, int start, int end, int cc, Pos3 &center, float &size) {
    // (four nodes' coordinates per trip, added in node order as before: a load per coordinate, each waited for, made this two memory
    // round trips per node of the cluster)
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (int u0 = start; u0 < end; u0 += 4) {
        float x[4], y[4], z[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t o = (uint32_t)(min(u0 + k, end - 1) * 3 * C + cc);
            x[k] = xyz[o], y[k] = xyz[o + C], z[k] = xyz[o + 2 * C];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = u0 + k < end;
            sx = in ? sx + x[k] : sx;
            sy = in ? sy + y[k] : sy;
            sz = in ? sz + z[k] : sz;
        }
    }
    const float cnt = (float)(end - start);
    center = Pos3{sx / cnt, sy / cnt, sz / cnt};
    float mx = 0.f;
    for (int u0 = start; u0 < end; u0 += 4) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t o = (uint32_t)(min(u0 + k, end - 1) * 3 * C + cc);
            r[k] = norm3f(xyz[o] - center.x, xyz[o + C] - center.y, xyz[o + 2 * C] - center.z);
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) mx = (u0 + k == start || (u0 + k < end && r[k] > mx)) ? r[k] : mx;
    }
    size = mx;
}

// The self / pair score tables of match_utils.py for the ligand whose levels are in LDS, into `rec`.
template <int G, bool EXACT, bool TAILS>
__device__ __forceinline__ void build_tables(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, const Record &r, const LevelInfo &L,
                                             unsigned char *rec, uint32_t &n_items, uint32_t &n_exact, uint32_t &n_exactv, uint32_t &n_dead) {
    constexpr int SLOTS = 64 / G;
    constexpr uint64_t GM = group_mask<G>();
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    const int C = r.C, cc = c < C ? c : C - 1;
    const uint8_t *lstart = lds + kOffStart, *lend = lds + kOffEnd, *lk = lds + kOffK;
    const uint16_t *ksum = reinterpret_cast<const uint16_t *>(lds + kOffKsum), *ncoff = reinterpret_cast<const uint16_t *>(lds + kOffNcoff);
    const uint8_t *cand = lds + ws.off_cand, *lcnt = lds + ws.off_lcnt;
    const uint16_t *nc = reinterpret_cast<const uint16_t *>(lds + ws.off_nc);
    const uint32_t *rowbase_l = reinterpret_cast<const uint32_t *>(lds + kOffRow);
    GlobalFloats xyz = (GlobalFloats)uniptr(r.xyz);
    float *St = reinterpret_cast<float *>(rec + rec_s_off<G>());
    float *Pt = reinterpret_cast<float *>(rec + rec_p_off<G>(L.ksumtot));
    unsigned char *Vt = rec + rec_v_off<G>(L.ksumtot, L.T, (uint32_t)L.nl);
    const int nl = L.nl, K = p.M.K;
    // Node distances of the cluster (pair) in work, once, in LDS: every table entry of the pair - k_i k_j of them - reads the
    // distances of the same node pairs, and a distance from coordinates is six loads, each of which occupies the L1 for four
    // cycles whether or not its lanes share an address. The table phase was bound by exactly that (rocprofv3: 0.86 L1 accesses
    // per cycle and CU, 67 % of its wave cycles waiting on memory). The walker's LDS (children cache, level maxima) is idle
    // in this phase and holds 82 node pairs at 8 lanes; larger pairs - and the 32 / 64-lane shapes, which keep nothing
    // there - compute from the coordinates as before. (The cell of the distance staged with it - the same for every entry
    // too - halves what fits and costs more than it saves: measured.)
    constexpr uint32_t kPfBytes = 2u * G * 4u; // (the cluster distance and size sum of the level pair, below, come first)
    // At 32 / 64 lanes the wave's buffer of path totals in global memory (idle until the walk) takes their place: one coalesced
    // load per item instead of six and the square root.
    constexpr bool kStageLds = totals_in_lds<G>();
    float *dl = kStageLds ? reinterpret_cast<float *>(lds + ws.off_tch + kPfBytes) : reinterpret_cast<float *>(p.totbuf + (size_t)blockIdx.x * kTotBufBytes);
    const int dcap = kStageLds ? (int)((ws.bytes - ws.off_tch - kPfBytes) / (uint32_t)(G * 4)) : (int)(kTotBufBytes / (uint32_t)(G * 4));
#ifdef PMX_TABLE_TICKS
    unsigned long long tick_ = __builtin_amdgcn_s_memtime();
#endif
    auto node_distance = [&](int a0, int u, int b0, int v) {
        const uint32_t ou = (uint32_t)((a0 + u) * 3 * C + cc), ov = (uint32_t)((b0 + v) * 3 * C + cc);
        return norm3f(xyz[ou] - xyz[ov], xyz[ou + C] - xyz[ov + C], xyz[ou + 2 * C] - xyz[ov + 2 * C]);
    };
    auto stage_distances = [&](int a0, int na, int b0, int nb) { // dl[(u * nb + v) * G + c] = |x_(a0 + u) - x_(b0 + v)|
        lds_sync();                                              // (readers of the last pair's distances are done)
        const float inv_nb = 1.0f / (float)nb;
        for (int pr = s; pr < na * nb; pr += 2 * SLOTS) { // (two node pairs per trip: twelve coordinate loads in flight instead of six)
            const int pr2 = pr + SLOTS < na * nb ? pr + SLOTS : pr;
            const int u = (int)(((float)pr + 0.5f) * inv_nb), v = pr - u * nb;
            const int u2 = (int)(((float)pr2 + 0.5f) * inv_nb), v2 = pr2 - u2 * nb;
            const float d1 = node_distance(a0, u, b0, v), d2 = node_distance(a0, u2, b0, v2);
            dl[pr * G + c] = d1;
            dl[pr2 * G + c] = d2;
        }
        if (kStageLds) lds_sync();
        else wave_sync();
    };
    // Centre and size of every level's ligand cluster (ligand.py:458-473), once, with a slot per level: the pair loop below needs
    // them for every pair of levels and used to work them out again per pair (nl (nl - 1) / 2 + nl times instead of nl: 6 % of
    // the bench pass). They wait in the record's R / W regions, which build_bounds() fills only after this phase.
    constexpr bool kCentersStaged = cand_bounds<G>(); // (the W region exists; single-node clusters - the 32 / 64-lane stress model - gain nothing)
    float2 *cxy = reinterpret_cast<float2 *>(rec + rec_r_off<G>(L.ksumtot, L.T));
    float2 *czs = reinterpret_cast<float2 *>(rec + rec_w_off<G>(L.ksumtot, L.T, (uint32_t)L.nl));
    if (kCentersStaged) {
        for (int l = s; l < nl; l += SLOTS) {
            Pos3 ctr;
            float size;
            center_size(xyz, C, (int)lstart[l], (int)lend[l], cc, ctr, size);
            cxy[l * G + c] = make_float2(ctr.x, ctr.y);
            czs[l * G + c] = make_float2(ctr.z, size);
        }
        wave_sync();
    }
    for (int i = 0; i < nl; ++i) {
        const int si = uni(lstart[i]), ni = uni(lend[i]) - si, ki = uni(lk[i]), nci = uni(ncoff[i]), ksi = uni(ksum[i]);
        const uint32_t row_i = (uint32_t)uni((int)rowbase_l[i]), nd_i = L.ksumtot - (uint32_t)uni(ksum[i + 1]);
        // ---- self table S[i][a] (match_utils.py:77-122): node pairs u < v of the cluster
        const bool self_staged = !(PMX_CUT & 1) && ni >= PMX_SELF_STAGE_MIN && ni * ni <= dcap;
        if (self_staged) stage_distances(si, ni, si, ni);
        for (int q0 = 0; q0 < ki; q0 += SLOTS) {
            const int q = q0 + s;
            const bool on = q < ki;
            const int row = nci + (on ? q : 0) * ni;
            float acc = 0.f;
            int fails = 0;
            for (int u = 0; u + 1 < ((PMX_CUT & 1) ? 0 : ni); ++u) {
                const uint32_t sidu = nc[row + u];
                for (int v = u + 1; v < ni; ++v) {
                    const float d = self_staged ? dl[(u * ni + v) * G + c] : node_distance(si, u, si, v);
                    item<EXACT, true>(p, sidu, nc[row + v], d, acc, fails, n_exact, n_exactv);
                    ++n_items;
                }
            }
            if (on) St[(size_t)(ksi + q) * G + c] = acc;
        }
        PMX_TICK(0);
        Pos3 ctr_i;
        float size_i;
        if (kCentersStaged) {
            const float2 a = cxy[i * G + c], b = czs[i * G + c];
            ctr_i = Pos3{a.x, a.y, b.x};
            size_i = b.y;
        } else {
            center_size(xyz, C, si, si + ni, cc, ctr_i, size_i);
        }
        for (int j = i + 1; j < nl; ++j) {
            const int sj = uni(lstart[j]), nj = uni(lend[j]) - sj, kj = uni(lk[j]), ncj = uni(ncoff[j]);
            Pos3 ctr_j;
            float size_j;
            if (kCentersStaged) {
                const float2 a = cxy[j * G + c], b = czs[j * G + c];
                ctr_j = Pos3{a.x, a.y, b.x};
                size_j = b.y;
            } else {
                center_size(xyz, C, sj, sj + nj, cc, ctr_j, size_j);
            }
            const float ldist = norm3f(ctr_i.x - ctr_j.x, ctr_i.y - ctr_j.y, ctr_i.z - ctr_j.z); // graph_match.py:240
            const float lsize = size_i + size_j;                                                  // :241
            const int E = ki * kj;
            const float inv_kj = 1.0f / (float)kj;
            const uint32_t off_j = (uint32_t)(uni(ksum[j]) - uni(ksum[i + 1])); // (j's candidates inside the run of (i, a)'s entries)
            // Which entries pass the cluster-distance prefilter (graph_match.py:263-268: an entry is computed if some conformer
            // passes) is settled first, 64 entries at a time with the lanes spread over *entries* - for a model of 30-40 clusters
            // most of the k_i k_j entries of a level pair fail, and walking them eight at a time was most of the table phase.
            // Failing entries get their -1 row and empty mask right there; the passing ones are listed and computed eight at a time.
            float *pf = reinterpret_cast<float *>(lds + ws.off_tch); // [G] cluster distance | [G] size sum, per conformer
            uint8_t *plist = lds + ws.off_task;                      // passing entries of the chunk (the root record is written later)
            if (s == 0) {
                pf[c] = ldist;
                pf[G + c] = lsize;
            }
            const bool staged = ni * nj <= dcap;
            const bool dead_test = staged && ni <= 64 && nj <= 64 && !(PMX_WFLAGS(p) & 65536u);
            PMX_TICK(1);
            if (staged) stage_distances(si, ni, sj, nj);
            else lds_sync();
            PMX_TICK(2);
            for (int eb = 0; eb < E; eb += 64) {
                unsigned long long pbal;
                {
                    const int e = eb + lane;
                    const bool in = e < E;
                    const int ee = in ? e : eb;
                    const int sa = (int)(((float)ee + 0.5f) * inv_kj), sb = ee - sa * kj;
                    const float2 mp = p.M.cpair[cand[i * ws.kp + sa] * K + cand[j * ws.kp + sb]];
                    bool pass = false;
                    {   // (eight conformers per trip - lanes past C hold copies of conformer C - 1, which an OR does not mind: the reads of a trip are two wide LDS loads)
                        constexpr int KP = G < 8 ? G : 8;
                        for (int k0 = 0; k0 < C; k0 += KP) {
#pragma unroll
                            for (int kk = 0; kk < KP; ++kk) pass = pass || !((fabsf(pf[k0 + kk] - mp.x) - pf[G + k0 + kk]) > mp.y);
                        }
                    }
                    pass = pass && in;
                    // Dead entries. An entry that passes the prefilter is still -1 for every conformer when more than half of
                    // its counted node pairs fail the 2-sigma majority test (match_utils.py:55-61, :71-74) - for a pocket of 20-40
                    // clusters that is every second entry and every second item. A node pair whose distance lies outside the
                    // hull of the windows of ALL model node pairs of the two clusters (DevModel::cwin, exact float ends) passes no
                    // term, whatever the node subsets: it certainly fails. Counting those - two compares on a staged distance,
                    // no function cell - gives a lower bound cf on an entry's fails per conformer, and 2 cf > L1 L2 for every
                    // conformer settles the entry: its row is -1 and its mask empty, exactly what the items would have given.
                    // (Lanes over entries like the prefilter: C x pairs trips per 64 entries against pairs x 64 / SLOTS item trips.)
                    if (dead_test && E >= (int)p.dead_min_entries) {
                        const float2 w = p.M.cwin[cand[i * ws.kp + sa] * K + cand[j * ws.kp + sb]];
                        unsigned long long mu = 0ull, mv = 0ull; // nodes with a non-empty subset under the candidate (graph_match.py:164-171)
                        if (pass) {
                            const int rowa = nci + sa * ni, rowb = ncj + sb * nj;
                            for (int u = 0; u < ni; ++u) mu |= (unsigned long long)(nc[rowa + u] != 0 ? 1 : 0) << u;
                            for (int v = 0; v < nj; ++v) mv |= (unsigned long long)(nc[rowb + v] != 0 ? 1 : 0) << v;
                        }
                        const int L1L2 = (int)__popcll(mu) * (int)__popcll(mv);
                        bool dead = pass && L1L2 > 0;
                        constexpr int KB = G < 8 ? G : 8; // conformers per trip: their distances of a node pair are one batch of loads
                        for (int k0 = 0; k0 < C; k0 += KB) {
                            if (__ballot(dead) == 0ull) break;
                            int cf[KB];
#pragma unroll
                            for (int kk = 0; kk < KB; ++kk) cf[kk] = 0;
                            for (int u = 0; u < ni; ++u) {
                                const int bu = (int)(mu >> u) & 1;
                                for (int v = 0; v < nj; ++v) {
                                    const int on_uv = bu & (int)(mv >> v);
                                    const float *dp = dl + (u * nj + v) * G + k0; // (lanes of a slot past C hold copies of conformer C - 1)
#pragma unroll
                                    for (int kk = 0; kk < KB; ++kk) {
                                        const float d = dp[kk];
                                        cf[kk] += (on_uv & ((d < w.x || d > w.y) ? 1 : 0));
                                    }
                                }
                            }
#pragma unroll
                            for (int kk = 0; kk < KB; ++kk) dead = dead && 2 * cf[kk] > L1L2;
                        }
                        n_dead += (uint32_t)__popcll(__ballot(dead));
                        pass = pass && !dead;
                    }
                    pbal = __ballot(pass);
                    if (in && !pass) {
                        float *row = Pt + (size_t)(row_i + (uint32_t)sa * nd_i + off_j + (uint32_t)sb) * G;
                        if (G >= 4) {
#pragma unroll
                            for (int g = 0; g < G; g += 4) *reinterpret_cast<float4 *>(row + g) = make_float4(-1.f, -1.f, -1.f, -1.f);
                        } else {
                            for (int g = 0; g < G; ++g) row[g] = -1.f;
                        }
                        unsigned char *ve = Vt + (size_t)(row_i + (uint32_t)sa * nd_i + off_j + (uint32_t)sb) * vmask_bytes<G>();
                        for (uint32_t g = 0; g < vmask_bytes<G>(); ++g) ve[g] = 0;
                    }
                    if (pass) {
                        const uint32_t lo32 = (uint32_t)pbal, hi32 = (uint32_t)(pbal >> 32);
                        plist[__builtin_amdgcn_mbcnt_hi(hi32, __builtin_amdgcn_mbcnt_lo(lo32, 0u))] = (uint8_t)lane;
                    }
                }
                lds_sync();
                PMX_TICK(3);
                const int npass = (int)__popcll(pbal);
                // what is written for a finished entry: match_utils.py:71-74 (-1 unless num_fails <= L1 * L2 / 2), the row and its V mask
                auto finish_entry = [&](int e, bool on, float acc, int fails) {
                    const int sa = (int)(((float)e + 0.5f) * inv_kj), sb = e - __mul24(sa, kj);
                    const int L1 = lcnt[i * ws.kp + sa], L2 = lcnt[j * ws.kp + sb]; // graph_match.py:164-171
                    const float value = 2 * fails <= L1 * L2 ? acc : -1.f;
                    const uint32_t pe = row_i + __umul24((uint32_t)sa, nd_i) + off_j + (uint32_t)sb; // entry((i, sa) -> (j, sb)); sa < 64, nd_i <= 20 x 64
                    if (on) Pt[(size_t)pe * G + c] = value;
                    const unsigned long long pos = __ballot(on && value > 0.f);
                    if (on && c == 0) {
                        const unsigned long long m = (pos >> (s * G)) & GM;
                        unsigned char *ve = Vt + (size_t)pe * vmask_bytes<G>();
                        if (G <= 8) *ve = (unsigned char)m;
                        else if (G == 16) *reinterpret_cast<uint16_t *>(ve) = (uint16_t)m;
                        else if (G == 32) *reinterpret_cast<uint32_t *>(ve) = (uint32_t)m;
                        else *reinterpret_cast<unsigned long long *>(ve) = m;
                    }
                };
                if (EXACT) {
                    for (int p0 = 0; p0 < npass; p0 += SLOTS) {
                        const bool on = p0 + s < npass;
                        const int e = eb + (int)plist[on ? p0 + s : p0];
                        const int sa = (int)(((float)e + 0.5f) * inv_kj), sb = e - sa * kj;
                        float acc = 0.f;
                        int fails = 0;
                        const int rowa = nci + sa * ni, rowb = ncj + sb * nj;
                        for (int u = 0; u < ni; ++u) {
                            const uint32_t sidu = nc[rowa + u];
                            for (int v = 0; v < nj; ++v) {
                                const float d = staged ? dl[(u * nj + v) * G + c] : node_distance(si, u, sj, v);
                                item<EXACT, false>(p, sidu, nc[rowb + v], d, acc, fails, n_exact, n_exactv);
                            }
                        }
                        finish_entry(e, on, acc, fails);
                    }
                    n_items += (uint32_t)(((npass + SLOTS - 1) / SLOTS) * ni * nj);
                } else if constexpr (SLOTS == 1) {
                    // 64 conformer lanes: the wavefront works on ONE entry at a time, so nothing forces it through the node pairs that
                    // count for nothing - a node whose subset under the candidate is empty (graph_match.py:148-155: no model node of its
                    // types in the cluster) adds 0 and never fails, and 45 % of the stress model's items are such pairs. (With 8 slots
                    // the slots walk in step, and a pair that is empty for one entry is not for its neighbours.) The items of the chunk
                    // are one list as below - entries in turn, of each its counted pairs in the reference's order, PMX_ITEM_BATCH cells on
                    // the way at a time across entry boundaries - over L1 x L2 pairs per entry instead of all of them.
                    constexpr int IB = PMX_ITEM_BATCH;
                    int total = 0, npass2 = 0;
                    {
                        const bool inl = lane < npass;
                        const int el = plist[inl ? lane : 0];
                        const int e = eb + el;
                        const int sa = (int)(((float)e + 0.5f) * inv_kj), sb = e - sa * kj;
                        int cnt = inl ? (int)lcnt[i * ws.kp + sa] * (int)lcnt[j * ws.kp + sb] : 0;
                        if (inl && cnt == 0) { // no counted pair: the sum of nothing, no fails (match_utils.py:71-74): 0 for every conformer, empty mask
                            const uint32_t pe = row_i + (uint32_t)sa * nd_i + off_j + (uint32_t)sb;
                            float *row = Pt + (size_t)pe * G;
#pragma unroll
                            for (int g = 0; g < G; g += 4) *reinterpret_cast<float4 *>(row + g) = make_float4(0.f, 0.f, 0.f, 0.f);
                            unsigned char *ve = Vt + (size_t)pe * vmask_bytes<G>();
                            for (uint32_t g = 0; g < vmask_bytes<G>(); ++g) ve[g] = 0;
                        }
                        const unsigned long long hb = __ballot(inl && cnt > 0);
                        lds_sync(); // (every lane has read its entry: the list is compacted in place)
                        if (inl && cnt > 0) plist[__builtin_amdgcn_mbcnt_hi((uint32_t)(hb >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)hb, 0u))] = (uint8_t)el;
                        npass2 = (int)__popcll(hb);
#pragma unroll
                        for (int d = 1; d < 64; d <<= 1) cnt += __shfl_xor(cnt, d);
                        total = uni(cnt);
                    }
                    lds_sync();
                    int le = -1, lu = 0, rowa = 0, rowb = 0;
                    unsigned long long mur = 0ull, mvr = 0ull, mv_full = 0ull; // nodes of the two clusters still to come for the entry being loaded
                    auto counted = [&](int k) { // L1 x L2 of the k-th listed entry
                        const int e = eb + uni((int)plist[k]);
                        const int sa = (int)(((float)e + 0.5f) * inv_kj), sb = e - sa * kj;
                        return uni((int)lcnt[i * ws.kp + sa]) * uni((int)lcnt[j * ws.kp + sb]);
                    };
                    int fk = 0, fin_left = npass2 > 0 ? counted(0) : 0;
                    float acc = 0.f;
                    int fails = 0;
                    for (int t0 = 0; t0 < total; t0 += IB) {
                        ItemLoad Lq[IB];
#pragma unroll
                        for (int q = 0; q < IB; ++q) {
                            const bool in = t0 + q < total; // (past the end: the empty subset pair)
                            int lv = 0;
                            if (in) {
                                if (mvr == 0ull) {
                                    mur &= mur - 1ull; // the next node of the first cluster (0 stays 0)
                                    if (mur == 0ull) { // the next entry
                                        ++le;
                                        const int e = eb + uni((int)plist[le]);
                                        const int sa = (int)(((float)e + 0.5f) * inv_kj), sb = e - sa * kj;
                                        rowa = nci + sa * ni, rowb = ncj + sb * nj;
                                        mur = __ballot(lane < ni && nc[rowa + (lane < ni ? lane : 0)] != 0);
                                        mv_full = __ballot(lane < nj && nc[rowb + (lane < nj ? lane : 0)] != 0);
                                    }
                                    lu = __ffsll((unsigned long long)mur) - 1;
                                    mvr = mv_full;
                                }
                                lv = __ffsll((unsigned long long)mvr) - 1;
                                mvr &= mvr - 1ull;
                            }
                            const int uu = in ? lu : 0, vv = in ? lv : 0;
                            const float d = staged ? dl[(uu * nj + vv) * G + c] : node_distance(si, uu, sj, vv);
                            Lq[q] = item_load(p, in ? (uint32_t)nc[rowa + uu] : 0u, in ? (uint32_t)nc[rowb + vv] : 0u, d, cell_of(p, d));
                        }
#pragma unroll
                        for (int q = 0; q < IB; ++q) {
                            if (t0 + q < total) {
                                item_finish<TAILS>(p, Lq[q], acc, fails, n_exact, n_exactv);
                                if (--fin_left == 0) {
                                    finish_entry(eb + uni((int)plist[fk]), true, acc, fails);
                                    acc = 0.f, fails = 0;
                                    if (++fk < npass2) fin_left = counted(fk);
                                }
                            }
                        }
                    }
                    n_items += (uint32_t)total;
                } else {
                    // The (entry, node pair) items of the chunk as ONE list per slot - slot s takes the passing entries s, s + SLOTS, ...
                    // and every entry its node pairs (u, v) in the reference's order (u outer) - walked PMX_ITEM_BATCH items at a
                    // time: coordinates, distances and cell loads of a batch go out together, whichever entries they belong to,
                    // then the values are added in order and an entry is written when its last pair is in. (With a batch per
                    // entry, entries of one or three node pairs - single-node clusters: most of a large model's - spent half
                    // of every batch on padding, and at 32 / 64 conformer lanes, one entry per pass, nothing overlapped at all.)
                    constexpr int IB = PMX_ITEM_BATCH;
                    const int npair = ni * nj;
                    const int nround = (npass + SLOTS - 1) / SLOTS;
                    const int total = nround * npair;
                    // (The loop is instantiated for staged / computed distances: what is fixed per level pair is decided once, not per
                    // item, and the list's end is tested per batch, not per item. [MI355X] tables alone 57.4 -> 56.7 ms per 1 M ligands.)
                    auto run_items = [&](auto staged_tag, auto tri_tag) {
                        constexpr bool STG = decltype(staged_tag)::value;
                        constexpr bool TRI = decltype(tri_tag)::value; // (false: nothing is known, the general index)
                        int lk = 0, lu = 0, lv = 0, lpos = 0; // next item to load: entry round, node pair, its number
                        int fk = 0, fr = 0;                   // next item to finish: entry round, pair number
                        int rowa = 0, rowb = 0;               // node-candidate rows of this slot's entry of round lk
                        auto slot_entry = [&](int k, bool &on) {
                            on = k * SLOTS + s < npass;
                            return eb + (int)plist[on ? k * SLOTS + s : k * SLOTS];
                        };
                        auto decode = [&](int k) {
                            bool on;
                            const int e = slot_entry(k, on);
                            const int sa = (int)(((float)e + 0.5f) * inv_kj);
                            const int sb = e - __mul24(sa, kj); // (entries, candidates and nodes are far below 2^23: 24-bit multiplies are full rate, 32-bit ones a quarter)
                            rowa = nci + __mul24(sa, ni), rowb = ncj + __mul24(sb, nj);
                        };
                        decode(0);
                        float acc = 0.f;
                        int fails = 0;
                        uint32_t sidu_cur = nc[rowa]; // (the first node's subset is read when the node changes, not per item)
                        auto load_next = [&]() {
                            const float d = STG ? dl[lpos * G + c] : node_distance(si, lu, sj, lv);
                            const ItemLoad L = TRI ? item_load_t<true>(p, sidu_cur, (uint32_t)nc[rowb + lv], d)
                                                   : item_load(p, sidu_cur, (uint32_t)nc[rowb + lv], d, cell_of(p, d));
                            ++lpos;
                            if (++lv == nj) {
                                lv = 0;
                                if (++lu == ni) {
                                    lu = 0, lpos = 0;
                                    if (++lk < nround) decode(lk);
                                }
                                sidu_cur = nc[rowa + lu];
                            }
                            return L;
                        };
                        auto finish_next = [&](const ItemLoad &L) {
                            item_finish<TAILS>(p, L, acc, fails, n_exact, n_exactv);
                            if (++fr == npair) {
                                bool on;
                                const int e = slot_entry(fk, on);
                                finish_entry(e, on, acc, fails);
                                fr = 0, ++fk;
                                acc = 0.f, fails = 0;
                            }
                        };
                        int t0 = 0;
                        for (; t0 + IB <= total; t0 += IB) { // whole batches: no test of the list's end inside
                            inject_valu<PMX_INJECT_VALU_ITEM>();
                            ItemLoad L[IB];
#pragma unroll
                            for (int q = 0; q < IB; ++q) L[q] = load_next();
#pragma unroll
                            for (int q = 0; q < IB; ++q) finish_next(L[q]);
                        }
                        for (; t0 < total; ++t0) finish_next(load_next()); // what is left of the list, one at a time
                    };
                    // (the triangular index where the distances are staged - nearly every item of nearly every model;
                    // two copies of the loop, not three: a table that is not triangular - a model whose edge matrix is not symmetric, which the
                    // reference cannot make - takes the general loop, which computes its distances; the kernel is 63 KB beside a 64 KB instruction cache)
                    if (PMX_CUT & 4) {
                    } else if (staged && p.F.tri) run_items(std::true_type{}, std::true_type{});
                    else run_items(std::false_type{}, std::false_type{});
                    n_items += (uint32_t)total;
#ifdef PMX_TABLE_FILL
                    if (lane == 0) {
                        reinterpret_cast<WaveStats *>(lds + ws.off_stat)->dbg[1] += (unsigned long long)total;
                        reinterpret_cast<WaveStats *>(lds + ws.off_stat)->dbg[5] += (unsigned long long)(npass * npair);
                    }
#endif
                }
                lds_sync(); // (the list is rewritten by the next chunk)
                PMX_TICK(4);
            }
        }
    }
}

// DP[x] of the record (see its layout): levels from the last one up, the entries of a level's candidates with all deeper
// candidates - one contiguous run of V masks - read with the lanes spread over entries, the maxima taken in LDS (the walker's
// children cache is idle here). A ligand with more candidates than that holds gets 255 everywhere: nothing is ruled out.
template <int G>
__device__ __forceinline__ void chain_lengths(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, const LevelInfo &L, unsigned char *rec) {
    const int lane = lane_id();
    const uint8_t *lk = lds + kOffK;
    const uint16_t *ksum = reinterpret_cast<const uint16_t *>(lds + kOffKsum);
    const uint32_t *rowbase = reinterpret_cast<const uint32_t *>(lds + kOffRow);
    const unsigned char *Vt = rec + rec_v_off<G>(L.ksumtot, L.T, (uint32_t)L.nl);
    unsigned char *DPt = rec + rec_dp_off<G>(L.ksumtot, L.T, (uint32_t)L.nl);
    // (32 / 64 conformer lanes keep next to nothing in LDS: there the lengths are worked out in the wave's buffer of path totals in
    // global memory, idle until the walk)
    constexpr bool kInLds = totals_in_lds<G>();
    uint32_t *dpl = kInLds ? reinterpret_cast<uint32_t *>(lds + ws.off_tch) : reinterpret_cast<uint32_t *>(p.totbuf + (size_t)blockIdx.x * kTotBufBytes);
    const uint32_t cap = kInLds ? (ws.bytes - ws.off_tch) / 4u : kTotBufBytes / 4u;
    if (L.ksumtot > cap || (PMX_WFLAGS(p) & (4u | 32768u))) {
        for (uint32_t x = (uint32_t)lane; x < L.ksumtot; x += 64u) DPt[x] = 255;
        return;
    }
    auto sync = [&]() {
        if (kInLds) lds_sync();
        else wave_sync();
    };
    sync();
    for (uint32_t x = (uint32_t)lane; x < L.ksumtot; x += 64u) dpl[x] = 1u;
    constexpr uint32_t VB = vmask_bytes<G>();
    for (int j = L.nl - 2; j >= 0; --j) {
        sync(); // (the deeper levels' lengths are final)
        const uint32_t kj = (uint32_t)uni(lk[j]), ksj = (uint32_t)uni((int)ksum[j]), ks1 = (uint32_t)uni((int)ksum[j + 1]);
        const uint32_t nd = L.ksumtot - ks1, row = (uint32_t)uni((int)rowbase[j]);
        const float inv_nd = 1.0f / (float)nd;
        for (uint32_t e0 = (uint32_t)lane; e0 < kj * nd; e0 += 256u) { // (four masks per lane and trip: their loads in flight together)
            bool v[4];
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t e = min(e0 + 64u * u, kj * nd - 1u);
                const unsigned char *ve = Vt + (size_t)(row + e) * VB;
                if (VB == 1) v[u] = *ve != 0;
                else if (VB == 2) v[u] = *reinterpret_cast<const uint16_t *>(ve) != 0;
                else if (VB == 4) v[u] = *reinterpret_cast<const uint32_t *>(ve) != 0u;
                else v[u] = *reinterpret_cast<const unsigned long long *>(ve) != 0ull;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4u; ++u) {
                const uint32_t e = e0 + 64u * u;
                if (e < kj * nd && v[u]) {
                    const uint32_t a = (uint32_t)(((float)e + 0.5f) * inv_nd), xo = e - a * nd;
                    atomicMax(&dpl[ksj + a], dpl[ks1 + xo] + 1u);
                }
            }
        }
    }
    sync();
    for (uint32_t x = (uint32_t)lane; x < L.ksumtot; x += 64u) DPt[x] = (unsigned char)dpl[x];
    sync();
}

// Upper bounds for the tree search: level l can add at most
//   U[l][c] = max(0, max_b (S[l][b][c] + sum_{j < l} max(0, max_a P[(j, a), (l, b)][c])))
// to a conformer's total whatever is picked on the other levels, so R[f][c] = sum_{l >= f} U[l][c] bounds everything the
// levels f.. add. (The reported score only needs the per-conformer maximum over leaves, graph_match.py:103-109.)
template <int G>
__device__ __forceinline__ void build_bounds(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, const LevelInfo &L, unsigned char *rec) {
    constexpr int SLOTS = 64 / G;
    const int lane = lane_id();
    const int s = lane / G, c = lane % G;
    const uint8_t *lk = lds + kOffK;
    const uint16_t *ksum = reinterpret_cast<const uint16_t *>(lds + kOffKsum);
    const uint32_t *rowbase = reinterpret_cast<const uint32_t *>(lds + kOffRow);
    const float *St = reinterpret_cast<const float *>(rec + rec_s_off<G>());
    const float *Pt = reinterpret_cast<const float *>(rec + rec_p_off<G>(L.ksumtot));
    double *Rt = reinterpret_cast<double *>(rec + rec_r_off<G>(L.ksumtot, L.T));
    double *Wt = reinterpret_cast<double *>(rec + rec_w_off<G>(L.ksumtot, L.T, (uint32_t)L.nl));
    unsigned char *OBraw = rec + rec_ob_off<G>(L.ksumtot, L.T, (uint32_t)L.nl);
    // OB[i]: a bound, rounded up (bfloat16 where per-candidate bounds exist, float32 for the single row BF)
    auto ob_put = [&](size_t i, double v) {
        if (ob_elt_bytes<G>() == 2) reinterpret_cast<uint16_t *>(OBraw)[i] = bf16_up(float_up(v));
        else reinterpret_cast<float *>(OBraw)[i] = float_up(v);
    };
    unsigned char *LVt = rec + rec_ci_off<G>(L.ksumtot, L.T, (uint32_t)L.nl);
    const int nl = L.nl;
    // Round 6: the level maxima the base pass works out - MP[j][x] = max(0, max_a P[(j, a), x]) for a candidate x of a deeper level - are kept (in the
    // wave's path-sum buffer, idle until the walk) for the W pass below, which used to work every one of them out again per window of level j's
    // candidates: a loop over the level's candidates and a cross-slot maximum per deeper candidate ([MI355X] 5.4 of the table phase's 41.4 ms).
    float *MP = reinterpret_cast<float *>(p.pabuf + (size_t)blockIdx.x * p.pa_bytes);
    const bool mp_ok = cand_bounds<G>() && p.pabuf != nullptr && (uint64_t)nl * L.ksumtot * G * 4u <= (uint64_t)p.pa_bytes;
#ifdef PMX_TABLE_TICKS
    unsigned long long tick_ = __builtin_amdgcn_s_memtime();
#endif
    if (PMX_CUT & 2) return;
    chain_lengths<G>(p, lds, ws, L, rec);
    PMX_TICK(5);
    if (PMX_WFLAGS(p) & 4) { // debug: nothing is ever dropped
        for (int l = s; l <= nl; l += SLOTS) Rt[(size_t)l * G + c] = __builtin_inf();
        if (cand_bounds<G>())
            for (uint32_t e = s; e < L.ksumtot; e += SLOTS) Wt[(size_t)e * G + c] = __builtin_inf();
        return;
    }
    double suffix = 0.0;
    if (s == 0) Rt[(size_t)nl * G + c] = 0.0;
    for (int l = nl - 1; l >= 0; --l) {
        const int kl = uni(lk[l]), ksl = uni(ksum[l]);
        double u = 0.0;
        for (int b = s; b < kl; b += SLOTS) {
            // the levels above l from the nearest one up: what has been added when level j is reached is what (l, b) can add
            // apart from its pair entries with levels <= j - OB[j][(l, b)], path_bound()'s table
            double v = (double)St[(size_t)(ksl + b) * G + c];
            // (two levels above l per trip, eight entries of each in flight: a maximum does not mind the last candidate being read again where
            // fewer are left. One load at a time, each waited for, this loop was a memory round trip per candidate of every level above.)
            for (int j = l - 1; j >= 0; j -= 2) {
                const int j2 = j - 1; // (-1: level j is the last one)
                const int kj = uni(lk[j]), kj2 = j2 >= 0 ? uni(lk[j2]) : 0;
                const uint32_t nd_j = L.ksumtot - (uint32_t)uni((int)ksum[j + 1]), nd_j2 = L.ksumtot - (uint32_t)uni((int)ksum[j2 + 1]);
                const uint32_t e0 = (uint32_t)uni((int)rowbase[j]) + (uint32_t)(ksl - uni((int)ksum[j + 1])) + (uint32_t)b; // entry((j, 0) -> (l, b))
                const uint32_t e02 = j2 >= 0 ? (uint32_t)uni((int)rowbase[j2]) + (uint32_t)(ksl - uni((int)ksum[j2 + 1])) + (uint32_t)b : e0;
                float m = 0.f, m2 = 0.f;
                for (int a0 = 0; a0 < max(kj, kj2); a0 += 8) {
                    float pv[8], pw[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        pv[u] = Pt[(size_t)(e0 + (uint32_t)min(a0 + u, kj - 1) * nd_j) * G + c];
                        pw[u] = j2 >= 0 ? Pt[(size_t)(e02 + (uint32_t)min(a0 + u, kj2 - 1) * nd_j2) * G + c] : 0.f;
                    }
#pragma unroll
                    for (int u = 0; u < 8; ++u) {
                        m = pv[u] > m ? pv[u] : m;
                        m2 = pw[u] > m2 ? pw[u] : m2;
                    }
                }
                if (cand_bounds<G>()) ob_put(((size_t)j * L.ksumtot + (size_t)(ksl + b)) * G + c, v);
                if (mp_ok) MP[((size_t)j * L.ksumtot + (size_t)(ksl + b)) * G + c] = m;
                v += (double)m;
                if (j2 >= 0) {
                    if (cand_bounds<G>()) ob_put(((size_t)j2 * L.ksumtot + (size_t)(ksl + b)) * G + c, v);
                    if (mp_ok) MP[((size_t)j2 * L.ksumtot + (size_t)(ksl + b)) * G + c] = m2;
                    v += (double)m2;
                }
            }
            if (cand_bounds<G>()) Wt[(size_t)(ksl + b) * G + c] = v; // base(l, b), replaced by the candidate's own bound below
            else ob_put((size_t)(ksl + b) * G + c, v);                 // BF: base(l, b) for path_bound_wide()
            if (c == 0) LVt[ksl + b] = (unsigned char)l;
            u = v > u ? v : u;
        }
#pragma unroll
        for (int d = G; d < 64; d <<= 1) {
            const double o = __shfl_xor(u, d);
            u = o > u ? o : u;
        }
        suffix += u;
        if (s == 0) Rt[(size_t)l * G + c] = suffix;
    }
    // W[(f, b)][c]: what the levels below f can add under a path whose newest match is (f, b) - as U, but with (f, b)'s own
    // pair entries instead of level f's maxima, over the candidates compatible with (f, b) only. Levels in ascending order:
    // the entries of the levels l > f still hold base(l, .).
    if (!cand_bounds<G>()) return; // one or two candidates per pass (32 / 64 conformers): the walker uses R
    wave_sync();
    // (the work below grows with windows^2 per level: with very many candidates it would cost more than the walk saves, and
    // every candidate gets its level's bound instead)
    uint32_t cost = 0;
    for (int f = 0; f < nl; ++f) {
        const uint32_t wf = ((uint32_t)uni(lk[f]) + SLOTS - 1) / SLOTS;
        cost += wf * wf * (L.ksumtot - (uint32_t)uni((int)ksum[f + 1]));
    }
    if ((PMX_WFLAGS(p) & 512) || cost > p.bound_cost) {
        for (int f = 0; f < nl; ++f) {
            const int kf = uni(lk[f]), ksf = uni(ksum[f]);
            const double r = Rt[(size_t)(f + 1) * G + c];
            wave_sync();
            for (int b = s; b < kf; b += SLOTS) Wt[(size_t)(ksf + b) * G + c] = r;
        }
        return;
    }
    if (mp_ok) {
        // Slot s <-> candidate b = b0 + s of level f, alone with its own entries: for every deeper candidate x = (l, b1) its base with level f's
        // maximum taken out and (f, b)'s own entry put in - three loads and two additions - the largest per level, the levels added up. The same
        // numbers in the same order as the loop this replaces: the same W to the last bit.
        for (int f = 0; f < nl; ++f) {
            const int kf = uni(lk[f]), ksf = uni(ksum[f]);
            const uint32_t x0 = (uint32_t)uni((int)ksum[f + 1]), nd_f = L.ksumtot - x0;
            const float *MPf = MP + (size_t)f * L.ksumtot * G;
            for (int b0 = 0; b0 < kf; b0 += SLOTS) {
                const int b = b0 + s;
                const float *Pb_ = Pt + ((size_t)(uint32_t)uni((int)rowbase[f]) + (size_t)(uint32_t)min(b, kf - 1) * nd_f) * G; // entry((f, b) -> x) = rowbase[f] + b nd_f + (x - x0)
                double acc = 0.0;
                for (int l = f + 1; l < nl; ++l) {
                    const int kl = uni(lk[l]), ksl = uni(ksum[l]);
                    double u = 0.0;
                    constexpr int B1 = 4; // (deeper candidates per trip, their loads in flight together; a maximum does not mind the last one being taken again)
                    for (int b10 = 0; b10 < kl; b10 += B1) {
                        double base[B1];
                        float mp[B1], pv[B1];
#pragma unroll
                        for (int q = 0; q < B1; ++q) {
                            const uint32_t x = (uint32_t)(ksl + min(b10 + q, kl - 1));
                            base[q] = Wt[(size_t)x * G + c];
                            mp[q] = MPf[(size_t)x * G + c];
                            pv[q] = Pb_[(size_t)(x - x0) * G + c];
                        }
#pragma unroll
                        for (int q = 0; q < B1; ++q) {
                            const double val = (base[q] - (double)mp[q]) + (double)pv[q];
                            u = (pv[q] > 0.f && val > u) ? val : u;
                        }
                    }
                    acc += u;
                }
                if (b < kf) Wt[(size_t)(ksf + b) * G + c] = acc * (1.0 + 1e-12);
            }
        }
        wave_sync();
        return;
    }
    // (no room for the maxima: every candidate gets its level's bound)
    for (int f = 0; f < nl; ++f) {
        const int kf = uni(lk[f]), ksf = uni(ksum[f]);
        const double r = Rt[(size_t)(f + 1) * G + c];
        wave_sync();
        for (int b = s; b < kf; b += SLOTS) Wt[(size_t)(ksf + b) * G + c] = r;
    }
}

// ------------------------------------------------------------------------------------------ kernels
// Bump allocation in the arena by lane 0; returns the byte offset (never 0: offset 0 means "not in the arena") or ~0ull.
__device__ inline unsigned long long arena_alloc(const ScreenParams &p, uint32_t bytes) {
    unsigned long long off = 0;
    if ((threadIdx.x & 63) == 0) off = atomicAdd(&p.ctl->arena_top, (unsigned long long)((bytes + 255u) & ~255u)) + 256ull;
    off = uni64(off);
    return off + bytes <= p.arena_bytes ? off : ~0ull;
}

// A job of a wavefront is a subtree record: one taken from the queue (the ligand's tables are in the arena), or the root of
// a ligand whose tables this wave has just built (record in the wave's LDS, tables in its slice or in the arena).

// Ligand -> job: levels, tables, bounds, and the root's subtree record in LDS. Returns the ligand's record (slice or arena), or
// nullptr when the ligand is finished without a tree search (unsupported record, no candidates, tables too large for this pass).
template <int G, bool EXACT, bool TAILS>
__device__ __forceinline__ unsigned char *prepare_ligand(const ScreenParams &p, unsigned char *lds, const WaveShape<G> &ws, const uint32_t li, const uint32_t wave_id,
                                                         WaveStats *stat) {
    const int lane = lane_id();
    const int c = lane % G;
    Record r = parse_record(uniptr(p.lib.data + p.lib.offsets[p.first + li]));
    r.n = uni(r.n), r.C = uni(r.C), r.ncl = uni(r.ncl); // the record is the same for the whole wave: say so
    r.typemask = uniptr(r.typemask), r.cluster_end = uniptr(r.cluster_end), r.xyz = uniptr(r.xyz);
    if (p.mode == 0) {
        if (!record_supported(r)) {
            if (lane == 0) {
                put_score(p, li, __builtin_nan(""));
                if (p.status) p.status[li] = PMX_LIGAND_UNSUPPORTED;
            }
            return nullptr;
        }
        if (lane == 0 && p.status) p.status[li] = PMX_LIGAND_OK;
    }
    const unsigned long long t_a = __builtin_amdgcn_s_memtime();
    const LevelInfo L = scan_ligand<G>(p, lds, ws, r);
    if (L.nl < 0) { // a ligand cluster with more than PMX_MAX_LEVEL_CANDIDATES candidate clusters
        if (lane == 0) {
            put_score(p, li, __builtin_nan(""));
            if (p.status) p.status[li] = PMX_LIGAND_UNSUPPORTED;
        }
        return nullptr;
    }
    if (L.nl == 0) { // no ligand cluster has a candidate (graph_match.py:95-99)
        if (lane == 0) put_score(p, li, 0.0);
        return nullptr;
    }
    const uint64_t bytes64 = rec_bytes<G>(L.ksumtot, L.T, (uint32_t)L.nl);
    unsigned char *rec = p.slices + (size_t)wave_id * p.slice_bytes;
    uint32_t rec16 = 0;
    if (p.mode < 2) {
        if (bytes64 > p.slice_bytes) { // tables do not fit the slice: a later pass with larger slices (or the arena) takes this ligand
            if (lane == 0) {
                if (p.mode == 0) {
                    const uint32_t o = atomicAdd(&p.ctl->ovf_count, 1u);
                    if (o < p.list_cap) p.ovf_list[o] = li;
                    atomicAdd(&p.ctl->stats[wave_id & (kScreenStatShards - 1)][7], 1ull);
                } else {
                    const uint32_t o = atomicAdd(&p.ctl->carry_count, 1u);
                    if (o < p.list_cap) p.carry_list[o] = li;
                }
            }
            return nullptr;
        }
    } else {
        const bool fits = bytes64 < (1ull << 31) && bytes64 + 256ull <= p.arena_bytes;
        const unsigned long long off = fits ? arena_alloc(p, (uint32_t)bytes64) : ~0ull;
        if (off == ~0ull) {
            // No room. Tables larger than the whole arena are reported; otherwise the arena is full of other ligands' tables (it
            // is a bump allocator that empties between passes), which says nothing about this ligand: it is listed and taken
            // again by a later arena pass that starts empty, so that a score does not depend on what else is in the batch.
            if (lane == 0) {
                if (fits && p.retry_out) {
                    const uint32_t o = atomicAdd(&p.ctl->retry_count[p.retry_slot], 1u);
                    if (o < p.list_cap) p.retry_out[o] = li;
                } else {
                    put_score(p, li, __builtin_nan(""));
                    if (p.status) p.status[li] = PMX_LIGAND_TOO_LARGE;
                }
            }
            return nullptr;
        }
        rec = p.arena + off;
        rec16 = (uint32_t)(off >> 4);
    }
    // ---- header
    RecHeader *H = reinterpret_cast<RecHeader *>(rec);
    const uint8_t *lk = lds + kOffK;
    const uint16_t *ksum = reinterpret_cast<const uint16_t *>(lds + kOffKsum);
    const uint32_t *rowbase = reinterpret_cast<const uint32_t *>(lds + kOffRow);
    if (lane == 0) {
        H->lig = li;
        H->nl = (uint32_t)L.nl;
        H->T = L.T;
        H->ksumtot = L.ksumtot;
        H->bytes = (uint32_t)bytes64;
        H->C = (uint32_t)r.C;
        H->pad[0] = 0; // not (yet) registered for finalize_kernel
    }
    if (lane < L.nl) {
        H->k[lane] = lk[lane];
        H->rowbase[lane] = rowbase[lane];
    }
    if (lane <= L.nl) H->ksum[lane] = ksum[lane];
    if (lane < G) reinterpret_cast<unsigned long long *>(rec + sizeof(RecHeader))[lane] = 0ull;
    uint32_t n_items = 0, n_exact = 0, n_exactv = 0, n_dead = 0;
    const unsigned long long t_b = __builtin_amdgcn_s_memtime();
    build_tables<G, EXACT, TAILS>(p, lds, ws, r, L, rec, n_items, n_exact, n_exactv, n_dead);
    wave_sync();
    const unsigned long long t_c = __builtin_amdgcn_s_memtime();
    build_bounds<G>(p, lds, ws, L, rec);
    // ---- the root as a subtree record (in LDS): frame 0, no matches, every conformer, totals 0
    {
        unsigned char *tr = lds + ws.off_task;
        TaskRec *th = reinterpret_cast<TaskRec *>(tr);
        if (lane == 0) {
            th->rec16 = rec16;
            th->f0 = 0;
            th->nm = 0;
            th->pad = 0;
            th->mask = (r.C >= 64) ? ~0ull : ((1ull << r.C) - 1ull);
        }
        if (lane < G) reinterpret_cast<double *>(tr + sizeof(TaskRec))[c] = 0.0;
    }
    wave_sync();
    const unsigned long long t_d = __builtin_amdgcn_s_memtime();
    if (lane == 0) {
        stat->cyc_scan += t_b - t_a, stat->cyc_tables += t_c - t_b, stat->cyc_bounds += t_d - t_c;
        stat->items += n_items;
        stat->dead += n_dead;
    }
    if (n_exact) atomicAdd(&stat->exact, (unsigned long long)n_exact);
    if (n_exactv) atomicAdd(&stat->exactv, (unsigned long long)n_exactv);
    return rec;
}

__device__ inline void flush_wave_stats(const ScreenParams &p, const WaveStats *stat, uint32_t wave_id, unsigned long long alive) {
    unsigned long long *st = p.ctl->stats[wave_id & (kScreenStatShards - 1)];
    atomicAdd(st + 0, stat->frames);
    atomicAdd(st + 1, stat->passes);
    atomicAdd(st + 2, stat->over);
    atomicAdd(st + 3, stat->items);
    atomicAdd(st + 4, stat->exact);
    atomicMax(st + 5, stat->longest);
    atomicAdd(st + 6, stat->tasks);
    atomicAdd(st + 14, stat->overflow);
    atomicAdd(st + 15, stat->pad[0]);
    atomicAdd(st + 7, stat->pad[1] << 32);
    atomicAdd(st + 8, stat->cyc_scan);
    atomicAdd(st + 9, stat->cyc_tables);
    atomicAdd(st + 10, stat->cyc_bounds);
    atomicAdd(st + 11, stat->cyc_walk);
    atomicAdd(st + 12, alive);
    atomicAdd(st + 13, stat->exactv);
    atomicAdd(st + 22, stat->npath);
    atomicAdd(st + 23, stat->dbg[7]);
    atomicAdd(st + 24, stat->dead);
#if defined(PMX_COUNTERS) || defined(PMX_TABLE_TICKS) || defined(PMX_TABLE_FILL) || defined(PMX_WALK_TICKS)
    for (int i = 0; i < 6; ++i) atomicAdd(st + 16 + i, stat->dbg[i]);
#endif
}

} // namespace PMX_NS
