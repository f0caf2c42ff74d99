// pmx_screen.hip - the screening hot path on gfx950 (CDNA4, wave64): one wavefront scores one ligand from its packed
// record to its score. This file holds the kernels; what they are made of sits in four headers, each on top of the one before:
//   pmx_screen_layout.h   records, queue, control block, kernel parameters (host and device, namespace pmx: one type for every unit)
//   pmx_screen_lds.h      PMX_NS and a wave's LDS, the one layout a compile-time switch changes (host and device; sizes launches)
//   pmx_screen_tables.h   wave helpers, the pair-function builder, the table phase and the bounds, prepare_ligand
//   pmx_screen_walk.h     the walker, its bound tests, prepare_walk, run_job
// pmx_api.hip (namespace pmx) and pmx_screen_debug.hip (pmx_dbg) include this file; pmx_explain.hip (pmx_x), pmx_rows.hip (pmx_r) and
// pmx_pose_fit.hip (pmx_f) stop at the tables.
//
// Reference path: PharmacophoreModel._scoring -> GraphMatcher.run() (src/pmnet/scoring/graph_match.py:63-279,
// scoring/match_utils.py:9-122, scoring/tree.py:15-104); citations below are relative to /root/reference/src/pmnet.
//
// Lanes. A wavefront is 64 / G *slots* of G lanes; lane c of a slot is conformer c (G = 2^ceil(log2(max conformers)):
// 8 at BASELINE.json's 8-conformer shape). What a slot stands for changes with the phase:
//   * table phase: a slot owns one table entry - (ligand cluster i, model cluster a) for the self table S, ((i, a), (j, b))
//     for the pair table P - and walks that entry's ligand node pairs (u, v) in a wave-uniform loop. The sum over the
//     compatible model node pairs of one (u, v),
//         F(d) = 1 / (|A||B|) * sum_{m in A, n in B} w_m w_n / std_mn * exp(-((d - mean_mn) / std_mn)^2 / 2),
//     depends on the ligand only through the scalar d = |x_u - x_v|: it is a property of the model (and the call's type
//     weights). fn_build_kernel tabulates every such F once per (model, weights) as piecewise quintic Hermite cells (from
//     F, F', F'' evaluated in float64 at the knots; measured deviation from the exact sum < 3e-9 of the function's peak at
//     h <= std_min / 5), so that an item costs one 32-byte gather and five FMAs instead of |A||B| (27 on average, up to
//     169) Gaussian terms. The discrete part of match_utils.py - `num_pass < num_match * 0.5` (:61) - is NOT approximated:
//     the set of distances where at least half of the model node pairs lie within 2 sigma is a union of float intervals
//     computed exactly on the host when the model is created (pmx_model_tables.cpp, cell_windows) and stored with the cells; cells
//     where that set is not one interval are flagged and counted term by term on the device. Cells whose polynomial is not
//     accurate relative to the function's own (tail) value are flagged too, and evaluated term by term in self entries
//     (FnCell, exact_value). The node distances of the cluster pair in work are staged once in LDS (build_tables).
//   * tree phase: ONE depth-first walker per wavefront with wave-uniform control (scalar registers, scalar branches);
//     a slot evaluates one candidate child of the current frame, so that a frame's children - their conformer
//     masks, float64 totals and bound tests - are one pass of independent loads. The walker's stack lives in lane-indexed
//     registers (v_readlane / v_writelane), the float64 path totals in 1.3 KB of LDS. Children are tested against a
//     per-candidate bound (build_bounds) and, before the walker enters one, against the bound its actual path gives
//     (path_bound): 60 frames per ligand on the bench library where the reference's search has 11 300 nodes.
//
// Memory. The score tables of a ligand (S, P, search bounds R / W / OB; 15 KB on average) are written to a per-wavefront slice of
// global memory and read back by the same wavefront: they stay in the CU's L1 / the XCD's L2 and are overwritten by the
// wave's next ligand - there is no per-chunk table arena, no size pass, no host read. Ligands whose tables exceed the
// slice, and trees that run over their budget, move to a bump-allocated arena: over-budget walkers append the open
// subtrees with >= 5 matches to a task queue (exactness argument: see walk()), which launches of task_kernel drain in rounds.
// Everything is ordered on the caller's stream.
#include "pmx_screen_walk.h"

// ---- tuning constants of this file (-D through tools/build_variant.py). No record or LDS layout depends on them, but the host planner in
// pmx_api.hip sizes launches from them: a variant compiles every unit that includes this file with the same values.
#ifndef PMX_SCREEN_WAVES
#define PMX_SCREEN_WAVES 6 // waves per SIMD the ligand kernel's register budget is set for (<= 80 VGPRs: nothing spilled to memory; [MI355X] 7: 72 VGPRs with 23 / 9 spilled, 121.5 against 117.9 ms per pass)
#endif
#ifndef PMX_TASK_WAVES
#define PMX_TASK_WAVES 6 // the same for the task kernel, the walker alone ([MI355X] 7: 71 VGPRs, nothing spilled, 107.5-108.8 against 106.7 ms per pass)
#endif

namespace PMX_NS {
using namespace pmx; // (pmx_device.h)

// Persistent wavefronts (one per block) over the ligands of a pass: build a ligand's tables in the wave's slice (modes 0 / 1)
// or in the arena (mode 2), walk its tree, write its score. A tree that runs over its budget hands its open subtrees to the
// task queue, which task_kernel drains afterwards. (One kernel for ligands and queued subtrees together was built: the two
// bodies in one loop cost 80-300 spilled registers, inside the walker's pass loop; apart they need none.)
template <int G, bool EXACT, bool TAILS>
__global__ __launch_bounds__(64, PMX_SCREEN_WAVES) void ligand_kernel(const ScreenParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane0 = lane_id();
    const uint32_t wave_id = blockIdx.x;
    const WaveShape<G> ws = wave_shape<G>(p.M.K, (int)p.max_nodes);
    const uint32_t todo = p.mode == 0 ? p.hi - p.lo
                          : min(p.mode == 1 ? p.ctl->ovf_count : (p.mode == 2 ? p.ctl->carry_count : p.ctl->retry_count[p.retry_slot ^ 1u]), p.list_cap);
    const uint32_t *list = p.mode == 1 ? p.ovf_list : (p.mode == 2 ? p.carry_list : p.retry_in);
    constexpr uint32_t kBatch = 1; // ligands claimed per atomic on the cursor
    WaveStats *stat = reinterpret_cast<WaveStats *>(lds + ws.off_stat);
    if (lane0 < (int)(sizeof(WaveStats) / 8)) reinterpret_cast<unsigned long long *>(stat)[lane0] = 0ull;
    wave_sync();
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    uint32_t lig_next = 0, lig_end = 0;
    for (;;) {
        const int lane = lane_id();
        if (lig_next == lig_end) {
            uint32_t base = 0;
            if (lane == 0) base = atomicAdd(&p.ctl->cursor[p.mode], kBatch);
            base = (uint32_t)uni((int)base);
            lig_next = min(base, todo);
            lig_end = min(base + kBatch, todo);
            if (lig_next == lig_end) break;
        }
        const uint32_t next = lig_next++;
        const uint32_t li = p.mode == 0 ? p.lo + next : (uint32_t)uni((int)list[next]);
        unsigned char *rec = prepare_ligand<G, EXACT, TAILS>(p, lds, ws, li, wave_id, stat);
        if (!rec) continue;
        const unsigned char *root = lds + ws.off_task;
        const uint32_t rec16 = (uint32_t)uni((int)reinterpret_cast<const TaskRec *>(root)->rec16);
        Walk<G> w;
        if (!(PMX_WFLAGS(p) & 16384) && prepare_walk<G>(p, lds, ws, root, rec, w)) run_job<G>(p, lds, ws, w, rec, rec16, false, wave_id, stat);
    }
    wave_sync();
    if (lane0 == 0) flush_wave_stats(p, stat, wave_id, __builtin_amdgcn_s_memtime() - t_start);
}

// Snapshot of the task queue between rounds: the records reserved since the last round are this round's subtrees. (Rounds are
// separate launches on purpose: what one wave queues has to be visible to waves on other XCDs, whose L2 is not coherent
// with the writer's inside a kernel - a queue drained by the kernel that fills it needs an L2 write-back per hand-over,
// measured at 15x the walk time.)
__global__ void round_kernel(Ctl *ctl, uint32_t qcap) {
    const int lane = threadIdx.x & 63;
    const uint32_t lo = ctl->round_hi[lane], hi = min(ctl->q_res[lane], qcap);
    uint32_t n = hi - lo, inc = n;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(inc, d);
        if (lane >= d) inc += t;
    }
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) n += __shfl_xor(n, d);
    ctl->round_lo[lane] = lo;
    ctl->round_hi[lane] = hi;
    ctl->round_inc[lane] = inc;
    if (lane == 0) {
        ctl->round_total = n;
        ctl->task_cursor = 0;
        for (int x = 0; x < 8; ++x) ctl->xcd_cursor[x][0] = 0;
    }
}

// Persistent wavefronts over the round's subtrees; a subtree that runs over its budget queues its own open subtrees for the
// next round (the last round's budget is unlimited).
template <int G>
__global__ __launch_bounds__(64, PMX_TASK_WAVES) void task_kernel(const ScreenParams p) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int lane0 = lane_id();
    const uint32_t wave_id = blockIdx.x;
    const uint32_t total = p.ctl->round_total;
    if (total == 0) return;
    const WaveShape<G> ws = wave_shape<G>(p.M.K, (int)p.max_nodes);
    WaveStats *stat = reinterpret_cast<WaveStats *>(lds + ws.off_stat);
    if (lane0 < (int)(sizeof(WaveStats) / 8)) reinterpret_cast<unsigned long long *>(stat)[lane0] = 0ull;
    wave_sync();
    const unsigned long long t_start = __builtin_amdgcn_s_memtime();
    // Task number -> (shard, record) through the inclusive counts round_kernel left. Shards 8x .. 8x + 7 (a contiguous range
    // of task numbers) belong to XCD x - block b runs on XCD b % 8 on this part, which only matters for speed: a wavefront
    // takes from its own group until it is empty, then from the next ones. (Nothing of this stays in registers over a walk.)
    uint32_t skip = 0;
    for (;;) {
        const int lane = lane_id();
        const uint32_t inc = p.ctl->round_inc[lane];
        uint32_t nx = 0xffffffffu;
        while (skip < 8) {
            const int xx = (int)((blockIdx.x + skip) & 7u);
            const uint32_t st = xx ? (uint32_t)rl((int)inc, 8 * xx - 1) : 0u, en = (uint32_t)rl((int)inc, 8 * xx + 7);
            if (st < en) {
                uint32_t cur = 0;
                if (lane == 0) cur = atomicAdd(&p.ctl->xcd_cursor[xx][0], 1u);
                cur = (uint32_t)uni((int)cur);
                if (cur < en - st) {
                    nx = st + cur;
                    break;
                }
            }
            ++skip;
        }
        if (nx == 0xffffffffu) break;
        const int sh = __popcll(__ballot(nx >= inc)); // shards wholly before task nx (inc is non-decreasing)
        const uint32_t before = sh ? (uint32_t)rl((int)inc, sh - 1) : 0u;
        const uint32_t recno = (uint32_t)uni((int)p.ctl->round_lo[sh]) + (nx - before);
        const unsigned char *tr = p.queue + ((size_t)sh * p.qcap + recno) * task_rec_bytes<G>();
        if (lane == 0) ++stat->tasks;
        unsigned char *rec = p.arena + (size_t)(uint32_t)uni((int)reinterpret_cast<const TaskRec *>(tr)->rec16) * 16;
        Walk<G> w;
        if (prepare_walk<G>(p, lds, ws, tr, rec, w)) run_job<G>(p, lds, ws, w, rec, (uint32_t)((rec - p.arena) >> 4), true, wave_id, stat);
    }
    wave_sync();
    if (lane0 == 0) flush_wave_stats(p, stat, wave_id, __builtin_amdgcn_s_memtime() - t_start);
}

// Scores of the ligands whose tree was split: mean over conformers of the combined maxima (graph_match.py:109).
template <int G>
__global__ void finalize_kernel(const ScreenParams p) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= min(p.ctl->heavy_count, p.list_cap)) return;
    const unsigned char *rec = p.arena + (size_t)p.heavy_list[i] * 16;
    const RecHeader *H = reinterpret_cast<const RecHeader *>(rec);
    const unsigned long long *best = reinterpret_cast<const unsigned long long *>(rec + sizeof(RecHeader));
    const int C = (int)H->C;
    double sum = 0.0;
    for (int c = 0; c < C; ++c) sum += __longlong_as_double((long long)best[c]);
    put_score(p, H->lig, sum / (double)C);
}

// In front of an arena pass over the ligands the last one had no room for: every subtree of the super-chunk is done and
// finalize has run, so the arena and the task queue start empty again.
__global__ void retry_prep_kernel(Ctl *ctl, uint32_t slot_out) {
    const int lane = threadIdx.x & 63;
    ctl->q_res[lane] = 0;
    ctl->round_lo[lane] = 0;
    ctl->round_hi[lane] = 0;
    if (lane == 0) {
        ctl->arena_top = 0;
        ctl->heavy_count = 0;
        ctl->cursor[3] = 0;
        ctl->retry_count[slot_out] = 0;
    }
}

// Start of a super-chunk: cursors, lists, arena and queue are empty again (the statistics survive unless asked).
__global__ void ctl_clear_kernel(Ctl *ctl, int clear_stats) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t head_words = offsetof(Ctl, stats) / 4, all_words = sizeof(Ctl) / 4;
    uint32_t *w = reinterpret_cast<uint32_t *>(ctl);
    if (i < head_words) {
        if (i != offsetof(Ctl, qflag) / 4) w[i] = 0;
        else if (clear_stats) w[i] = 0;
    } else if (i < all_words && clear_stats) {
        w[i] = 0;
    }
}

// Wave-wide reductions in front of statistics atomics: one atomic per wavefront instead of one per lane on the same
// address (device-scope atomics on one address serialise at some 20 ns each on this part; inactive lanes contribute 0).
__device__ inline unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ inline unsigned long long wave_max(unsigned long long v) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const unsigned long long o = __shfl_xor(v, d);
        v = o > v ? o : v;
    }
    return v;
}

// -------------------------------------------------------------------------------- library stats
// Also validates every record (a truncated or corrupt library must not make the scoring kernels read out of bounds): the
// header-implied size has to fit the record's byte range, cluster ends have to be monotonic and <= n_nodes, type masks
// <= 127. A record that fails is neutralised in the device copy (header zeroed -> PMX_LIGAND_UNSUPPORTED, score NaN) and
// counted; offsets that are not multiples of 16 or run backwards make the upload fail (out[5]).
__global__ void library_stats_kernel(DevLibrary lib, uint8_t *data_rw, uint64_t nbytes,
                                     unsigned long long *out /* [0] conformers [1] maxn [2] maxC [3] maxcl [4] unsupported [5] bad offsets [6] corrupt */) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long conf = 0, maxn = 0, maxc = 0, maxcl = 0, unsupported = 0, bad_offsets = 0, corrupt = 0;
    if (i < lib.n) {
        const uint64_t o0 = lib.offsets[i], o1 = lib.offsets[i + 1];
        if ((o0 & 15) || o1 < o0 + 8 || o1 > nbytes) {
            bad_offsets = 1;
        } else {
            Record r = parse_record(lib.data + o0);
            const uint64_t need = ((8ull + (uint64_t)r.n + (uint64_t)r.ncl + 3ull) & ~3ull) + 12ull * (uint64_t)r.n * (uint64_t)r.C;
            bool ok = need <= o1 - o0;
            if (ok && record_supported(r)) {
                int prev = 0;
                for (int q = 0; q < r.ncl && ok; ++q) {
                    const int e = r.cluster_end[q];
                    ok = e >= prev && e <= r.n;
                    prev = e;
                }
                for (int u = 0; u < r.n && ok; ++u) ok = r.typemask[u] < 128;
            }
            if (!ok) { // neutralise: 0 nodes, 0 conformers, 0 clusters
                *reinterpret_cast<uint64_t *>(data_rw + o0) = 0ull;
                corrupt = 1;
                unsupported = 1;
            } else {
                conf = (unsigned long long)r.C;
                maxn = (unsigned long long)r.n;
                maxc = (unsigned long long)r.C;
                maxcl = (unsigned long long)r.ncl;
                if (!record_supported(r)) unsupported = 1;
            }
        }
    }
    // one set of atomics per wavefront, not per ligand
    conf = wave_sum(conf);
    maxn = wave_max(maxn);
    maxc = wave_max(maxc);
    maxcl = wave_max(maxcl);
    unsupported = wave_sum(unsupported);
    bad_offsets = wave_sum(bad_offsets);
    corrupt = wave_sum(corrupt);
    if ((threadIdx.x & 63) == 0) {
        if (conf) atomicAdd(&out[0], conf);
        if (maxn) atomicMax(&out[1], maxn);
        if (maxc) atomicMax(&out[2], maxc);
        if (maxcl) atomicMax(&out[3], maxcl);
        if (unsupported) atomicAdd(&out[4], unsupported);
        if (bad_offsets) atomicAdd(&out[5], bad_offsets);
        if (corrupt) atomicAdd(&out[6], corrupt);
    }
}

} // namespace PMX_NS
