// pmx_screen_layout.h - what the host planner and the kernels of the screening path agree on, and nothing else: the tabulated pair
// functions (FnCell, FnTable), a ligand's table record (RecHeader, rec_*_off), the task queue (TaskRec), the control block (Ctl), the
// kernels' parameters (ScreenParams) and the fixed part of a wavefront's LDS (kOff*). Host and device; no kernel and no device helper
// lives here. plan_pocket (pmx_api.hip) sizes its buffers from these; pmx_screen_lds.h and pmx_screen_tables.h build on them.
//
// Everything here is in the fixed namespace pmx: the screening kernels are compiled several times, each into a namespace of its own
// (PMX_NS, pmx_screen_lds.h), and all of them, their launchers and the host planner pass ONE ScreenParams, one Ctl, one RecHeader. What makes
// that sound is a rule: this file holds no #if, #ifdef or #ifndef on a tuning or debug macro, so no two units of one library can see
// these layouts differently. The one layout that does depend on a switch (WaveShape, through PMX_TC_LEVELS) lives in pmx_screen_lds.h,
// per PMX_NS.
#pragma once
#include "pmx_device.h"

#pragma clang fp contract(off)

#define PMX_SCORES_F64 (1u << 30) // ScreenParams::flags: `scores` is a double array (pmx_score_f64); set by the host, not by PMX_TREE_FLAGS
#define PMX_PRODUCT_FLAGS (2u | 16384u) // the PMX_TREE_FLAGS switches libpmx's own kernels know (PMX_WFLAGS, pmx_screen_lds.h)

namespace pmx {
// One cell of a tabulated pair function: value(t) = c0 + t (c1 + t (c2 + t (c3 + t (c4 + t c5)))), t in [0, 1) the position
// inside the cell; the item passes the 2-sigma majority test of match_utils.py:56-61 iff lo <= d <= hi (lo = NaN: the pass
// set is not an interval inside this cell - count the terms).
// The lowest mantissa bit of c[5] is a flag: the polynomial is not accurate *relative to the function's own value* in this
// cell (the far tails of the Gaussians, and the last cell, which stands for every distance beyond the grid). Entries of the
// self table have no majority test (match_utils.py:77-122), so a self entry can consist of tail values only and be a
// ligand's whole score: the self loop evaluates the terms of a flagged cell one by one, in the reference's float32
// operations (exact_value). A pair entry that counts at all holds items that passed the 2-sigma majority test - values near
// the functions' peaks, next to which a tail value's error is below float32 rounding - and ignores the flag.
struct FnCell {
    float c[6];
    float lo, hi;
};
static_assert(sizeof(FnCell) == 32, "FnCell layout");

struct FnTable {
    const FnCell *cells; // two planes of float4[functions][ncell]: {c0, c1, c2, c3} | {c4, c5, lo, hi} (plane B = plane A + plane16 float4s):
                         // the eight conformers of a slot read neighbouring cells, and 16 bytes per cell and plane keep them in one cache line
    uint32_t plane16;
    uint32_t NS;         // node subsets (0 = empty)
    uint32_t ncell;
    float inv_h;
    uint32_t tri;        // the functions of a symmetric model are stored once per unordered subset pair
};

// Header of one ligand's tables, in a wave's slice or in the arena:
//   [RecHeader][best u64[G]][S float[ksumtot][G]][P float[T][G]][R double[nl + 1][G]][W double[ksumtot][G]][V mask[T]]
//   [OB bfloat16[nl][ksumtot][G]][LV u8[ksumtot]][DP u8[ksumtot]]                 (where per-candidate bounds exist, cand_bounds(); at
//   32 / 64 lanes there is no W, and OB is the one row BF float[ksumtot][G], see ob_rows())
// OB[f][x] for a candidate x = (l, b') of a level l > f: S[l][b'] + sum_{f < j < l} max(0, max_a P[(j, a), (l, b')]), rounded up - what
// (l, b') can add to a leaf total apart from its pair entries with the matches on the path down to level f (path_bound()).
// LV[x] = the level of candidate x.
// DP[x] = the longest chain of candidates of ascending levels that starts with x and in which every candidate has an entry
// with some conformer > 0 against the one before it (V != 0): no path through x holds more matches from x on (probe()).
// V[e] = the conformers c with P[e][c] > 0 (one bit per conformer, max(G, 8) / 8 bytes per entry): what decides which
// children of a tree node exist (tree.py:78-84), read with the lanes spread over candidates.
// Pair entry of (i, a) with a candidate x = ksum[j] + b of a deeper level j: rowbase[i] + a * nd_i + (x - ksum[i + 1]), nd_i = ksumtot -
// ksum[i + 1] the candidates below level i: the entries of (i, a) with ALL deeper candidates are one contiguous run, so the row of a
// match on the path against any deeper candidate x is (a number fixed per match) + x - what the walker's passes and path_bound() read.
struct RecHeader {
    uint32_t lig; // ligand index relative to the call's `first`
    uint32_t nl, T, ksumtot;
    uint32_t bytes; // of the whole record
    uint32_t C;
    uint32_t pad[2];
    uint8_t k[PMX_MAX_LEVELS];
    uint8_t pad2[12];
    uint16_t ksum[PMX_MAX_LEVELS + 4];
    uint32_t rowbase[PMX_MAX_LEVELS];
    uint8_t pad3[64];
};
static_assert(sizeof(RecHeader) == 256, "RecHeader layout");

template <int G>
__host__ __device__ constexpr uint32_t rec_s_off() {
    return sizeof(RecHeader) + G * 8;
}
template <int G>
__host__ __device__ inline uint32_t rec_p_off(uint32_t ksumtot) {
    return rec_s_off<G>() + (uint32_t)round16((uint64_t)ksumtot * G * 4);
}
template <int G>
__host__ __device__ inline uint32_t rec_r_off(uint32_t ksumtot, uint32_t T) {
    return rec_p_off<G>(ksumtot) + (uint32_t)round16((uint64_t)T * G * 4);
}
template <int G>
__host__ __device__ constexpr uint32_t vmask_bytes() {
    return G < 8 ? 1u : (uint32_t)G / 8u;
}
template <int G>
__host__ __device__ inline uint32_t rec_w_off(uint32_t ksumtot, uint32_t T, uint32_t nl) {
    return rec_r_off<G>(ksumtot, T) + (nl + 1u) * G * 8u;
}
// (per-candidate bounds exist where a pass holds >= 4 candidates: 1 .. 16 conformer lanes; see build_bounds)
template <int G>
__host__ __device__ constexpr bool cand_bounds() {
    return 64 / G >= 4;
}
// An upper bound needs little precision where it is only compared with: the OB rows of path_bound() are bfloat16 rounded up
// ([MI355X] 99.7 -> 98.3 ms per pass against float32, 200.6 -> 184.9 KB per ligand across the L2 <-> fabric boundary). W stays a float64:
// the walker adds it to float64 totals in every pass. BF, the single row of the 32 / 64-lane shapes, is a float32 rounded up.
template <int G>
__host__ __device__ constexpr uint32_t ob_elt_bytes() {
    return cand_bounds<G>() ? 2u : 4u;
}
// bytes of the W region: a double per candidate and conformer where per-candidate bounds exist, nothing otherwise. Until build_bounds()
// writes W, build_tables() parks the cluster centres there (float2[nl][G], as many bytes as nl rows of W): they fit because every level
// has at least one candidate, ksumtot >= nl.
template <int G>
__host__ __device__ inline uint32_t rec_w_bytes(uint32_t ksumtot) {
    return cand_bounds<G>() ? ksumtot * G * 8u : 0u;
}
template <int G>
__host__ __device__ inline uint32_t rec_v_off(uint32_t ksumtot, uint32_t T, uint32_t nl) {
    return rec_w_off<G>(ksumtot, T, nl) + rec_w_bytes<G>(ksumtot);
}
template <int G>
__host__ __device__ inline uint32_t rec_ob_off(uint32_t ksumtot, uint32_t T, uint32_t nl) {
    return rec_v_off<G>(ksumtot, T, nl) + (uint32_t)round16((uint64_t)T * vmask_bytes<G>());
}
// rows of the OB table: one per level where per-candidate bounds exist; ONE otherwise (32 / 64 conformer lanes) - BF[x] = base(x)
// rounded up, what candidate x can add to a leaf total at most whatever is matched above it (path_bound_wide())
template <int G>
__host__ __device__ constexpr uint32_t ob_rows(uint32_t nl) {
    return cand_bounds<G>() ? nl : 1u;
}
template <int G>
__host__ __device__ inline uint32_t rec_ci_off(uint32_t ksumtot, uint32_t T, uint32_t nl) {
    return rec_ob_off<G>(ksumtot, T, nl) + (uint32_t)round16((uint64_t)ob_rows<G>(nl) * ksumtot * G * ob_elt_bytes<G>());
}
template <int G>
__host__ __device__ inline uint64_t rec_bytes(uint32_t ksumtot, uint32_t T, uint32_t nl) {
    return (uint64_t)rec_s_off<G>() + round16((uint64_t)ksumtot * G * 4) + round16((uint64_t)T * G * 4) + (uint64_t)(nl + 1) * G * 8 +
           (uint64_t)rec_w_bytes<G>(ksumtot) + round16((uint64_t)T * vmask_bytes<G>()) +
           round16((uint64_t)ob_rows<G>(nl) * ksumtot * G * ob_elt_bytes<G>()) + 2 * round16((uint64_t)ksumtot);
}
// (DP u8[ksumtot] follows LV: rec_ci_off + round16(ksumtot))
template <int G>
__host__ __device__ inline uint32_t rec_dp_off(uint32_t ksumtot, uint32_t T, uint32_t nl) {
    return rec_ci_off<G>(ksumtot, T, nl) + (uint32_t)round16((uint64_t)ksumtot);
}

// A subtree handed to the task queue: its root has >= 5 matches (see walk()).
struct TaskRec { // 64 bytes, followed by double tot[G]
    uint32_t rec16; // arena offset of the ligand's record, in 16-byte units
    uint8_t f0;     // frame of the subtree's root
    uint8_t nm;     // matches on the path, root included
    uint16_t pad;
    uint64_t mask;                    // conformer mask of the root
    uint8_t path[2 * PMX_MAX_LEVELS]; // (level, candidate) of every match on the path
    uint32_t pad2[2];
};
static_assert(sizeof(TaskRec) == 64, "TaskRec layout");
template <int G>
__host__ __device__ constexpr uint32_t task_rec_bytes() {
    return sizeof(TaskRec) + G * 8;
}

constexpr int kShards = 64; // task queue shards (= the wave size: a task wave finds its record with one scan over the shards)
constexpr int kStatWords = 26;
constexpr int kScreenStatShards = 64;

// Device-side control block of one call (zeroed by ctl_clear_kernel at the start of every super-chunk).
// The task queue is kShards independent queues (shard s owns records [s * qcap, (s + 1) * qcap)): a device-scope atomic
// on one address is a serial resource on this multi-XCD part, and exports come by the million.
struct Ctl {
    uint32_t cursor[4];   // ligand cursors of the launches of a super-chunk: [0] slice pass, [1] large-slice pass, [2] arena pass
    uint32_t ovf_count;   // ligands whose tables do not fit a slice
    uint32_t carry_count; // ligands whose tables do not fit a large slice either
    uint32_t heavy_count; // records in the arena that finalize has to score
    uint32_t pad0;
    uint32_t retry_count[2]; // ligands of the arena pass that found the arena full (retried with the arena to themselves)
    uint32_t pad00[2];
    unsigned long long arena_top; // bump allocator (bytes)
    uint32_t qflag;               // a queue shard was full (the walker then keeps the subtree: exact, only slower)
    uint32_t pad1;
    uint32_t q_res[kShards];      // records reserved
    uint32_t round_lo[kShards], round_hi[kShards]; // the records of the current round (round_kernel)
    uint32_t round_total, task_cursor;
    uint32_t pad[2];
    uint32_t xcd_cursor[8][16];   // task cursors of the round, one per group of 8 shards (one 64-byte line each)
    uint32_t round_inc[kShards];  // records of the round in shards 0 .. s (task number -> shard)
    unsigned long long stats[kScreenStatShards][kStatWords]; // sharded: [0] frames [1] passes [2] walks over budget [3] items [4] exact-count cells [5] longest walk [6] tasks [7] slice overflows [8..12] phase ticks [13] self items evaluated term by term
};

// With 32 or 64 conformer lanes the float64 path totals (21 rows of G) are 5 / 11 KB: kept in LDS they cap the CU at 8 wavefronts.
// There they live in global memory (one buffer per wavefront, L1 / L2 resident), and the children cache - a frame of those
// shapes never has all its candidates in one pass - has no LDS at all.
constexpr uint32_t kTotBufBytes = 16384;
template <int G>
__host__ __device__ constexpr bool totals_in_lds() {
    return G < 32;
}
struct ScreenParams {
    DevModel M;
    FnTable F;
    DevLibrary lib;
    const uint16_t *sidtab;    // [K * 128] node subset of (model cluster, ligand type mask); 0 = empty
    const uint32_t *sub_off;   // [NS + 1] the model nodes of node subset s: sub_nodes[sub_off[s] .. sub_off[s + 1]), ascending (0 = the empty subset)
    const uint8_t *sub_nodes;
    Weights W;                 // for the exact-term debug path
    uint64_t first;            // library index of the call's first ligand
    uint32_t lo, hi;           // ligands [lo, hi) of the call (relative to first) are this super-chunk
    Ctl *ctl;
    uint8_t *totbuf;           // [waves][kTotBufBytes]: the path totals of the 32 / 64-lane shapes (LDS at fewer lanes)
    uint8_t *pabuf;            // [waves][pa_bytes]: path_bound()'s pair sums of the matches on the path, float[matches][ksumtot][G]
    uint32_t pa_bytes;
    uint8_t *slices;           // [waves][slice_bytes]
    uint32_t slice_bytes;
    uint8_t *arena;
    unsigned long long arena_bytes;
    uint32_t *ovf_list, *carry_list, *heavy_list; // ligand indices / arena offsets (16-byte units)
    uint32_t list_cap;
    uint8_t *queue;
    uint32_t qcap;             // records per shard
    uint32_t budget;           // passes after which a walker starts handing subtrees to the queue
    uint32_t min_levels;       // only subtrees with at least this many levels below their root are queued
    uint32_t flags;            // 2: never queue, 4: no bound test, 8: exact Gaussian terms instead of the tabulated functions, 32768: no chain lengths (probe()), 65536: no dead-entry test (build_tables), 131072: no path-aware test at 32 / 64 lanes (path_bound_wide())
    uint32_t max_nodes;        // of the library (sizes the LDS node tables)
    uint32_t last_round;       // task_kernel: never queue (walk every subtree to its end)
    uint32_t bound_cost; // per-candidate bounds are built when their cost estimate stays below this (build_bounds)
    uint32_t dead_min_entries; // the dead-entry test (build_tables) runs for level pairs with at least this many entries
    float *scores;             // float[count]; double[count] when flags & PMX_SCORES_F64 (put_score())
    int32_t *status;
    int mode;                  // 0: slice pass over [lo, hi); 1: large-slice pass over ovf_list; 2: arena pass over carry_list; 3: arena pass over retry_in
    const uint32_t *retry_in;  // mode 3: the ligands an earlier arena pass had no room for (count: ctl->retry_count[retry_slot ^ 1])
    uint32_t *retry_out;       // modes 2, 3: where such ligands go (count: ctl->retry_count[retry_slot]); nullptr: they are reported as too large
    uint32_t retry_slot;
};

// fixed part (512 bytes): tm[64] | lstart[20] lend[20] lk[20] pad[4] | ksum u16[24] | ncoff u16[24] | rowbase u32[20] | cand bits u64[20] | ksumtot, T | path staging u16[20]
constexpr uint32_t kOffTm = 0, kOffStart = 64, kOffEnd = 84, kOffK = 104, kOffKsum = 128, kOffNcoff = 176, kOffRow = 224, kOffBits = 304, kOffPath = 472;
static_assert(kOffBits + 8 * PMX_MAX_LEVELS + 8 <= kOffPath && kOffPath + 2 * PMX_MAX_LEVELS <= 512, "fixed LDS part");

} // namespace pmx
