// pmx_enrich.hip - retrospective validation on the device: pmx_enrichment (include/pmx.h holds the specification).
//
// A labelled list of actives and decoys, one or more columns of scores over it, and per column the integers and sums a host turns into
// AUROC, enrichment factors and BEDROC - for the sample itself (row 0) and for n_boot Poisson bootstrap resamples of it (rows 1 ...).
// Everything is enqueued on the caller's stream and nothing is read back:
//
//   totals_kernel   one work-group per row: N*, n_a*, n_d* of the row (the resample counts are a hash of (seed, row, ligand), so they
//                   are recomputed wherever they are needed and never stored)
//   per column:
//     keys_kernel   the rank key of every ligand: the order-preserving bit pattern of its score, inverted (ascending key = descending
//                   score), after the canonicalisation of the specification (-0 is +0; NaN and a non-zero status are -inf); a ligand that
//                   is not counted (label 2) gets the key after every real one, so the counted ligands are the first N' of the sorted list
//     (hipcub's stable radix sort of (key, ligand index) pairs)
//     ranked_kernel a byte per position of the sorted list: bit 0 the ligand is an active, bit 1 the position starts a tie group,
//                   bit 2 the ligand is counted; and the optional `order` output
//   walk_kernel     one work-group per (column, row): streams the column's ranked bytes and ligand indices in tiles of kEnrichTile
//                   positions. A tile is one block-wide scan of (group open since the last head: weight, active weight; list so far:
//                   weight, active weight) whose left operand is the carry of the tiles before it, so a tie group may span any number of
//                   tiles. A group is closed by the thread that meets the next group's head (the last one by thread 0 after the last
//                   tile): there u2, the straddled cutoffs and the group's exp term are formed. Integer sums are exact in any order;
//                   the exp terms are summed per thread in the order the thread meets them and then by a fixed tree: no atomics, the
//                   same bits from call to call.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cmath>
#include <cstdint>
#include <mutex>
#include <vector>

#include "pmx.h"
#include "pmx_device.h"

namespace {

constexpr int kThreads = 256;
constexpr int kItems = 8;                       // consecutive positions per thread and tile
constexpr int kTile = kThreads * kItems;        // PMX_ENRICH_TILE
static_assert(kTile == PMX_ENRICH_TILE, "include/pmx.h names the walk's tile");
constexpr int kWaves = kThreads / 64;

// floor(2^64 * P(Poisson(1) <= m)), m = 0 .. 20 (include/pmx.h; tests/test_enrichment_cpu.py recomputes it with `decimal`)
constexpr int kPoissonEntries = 21;
__constant__ uint64_t kPoissonCdf[kPoissonEntries] = {
    0x5e2d58d8b3bcdf1aull, 0xbc5ab1b16779be35ull, 0xeb715e1dc1582dc2ull, 0xfb23979734a252f1ull, 0xff1025f59174dc3dull, 0xffd90f3ba4055e19ull,
    0xfffa8b71fc72c913ull, 0xffff540c0914b3c9ull, 0xffffed1f4aa8f120ull, 0xfffffe216e641462ull, 0xffffffd4d85d3183ull, 0xfffffffc6da262b4ull,
    0xffffffffba12d178ull, 0xfffffffffb07c64cull, 0xffffffffffab8ea5ull, 0xfffffffffffabe22ull, 0xffffffffffffb11aull, 0xfffffffffffffba1ull,
    0xffffffffffffffc5ull, 0xfffffffffffffffdull, 0xffffffffffffffffull};

__host__ __device__ inline uint64_t mix64(uint64_t x) {
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    return x;
}

__host__ __device__ inline uint64_t row_key(uint64_t seed, uint32_t b) { return mix64(seed + 0x9E3779B97F4A7C15ull * (uint64_t)b); }

// The count of ligand i in the row whose key is rk: how many table entries are <= h. Three in four draws are settled by the first
// two entries; the tail of the table is walked by the one draw in fifty that passes the fourth.
__device__ inline uint32_t poisson1(uint64_t rk, uint32_t i) {
    const uint64_t h = mix64(rk + (uint64_t)i);
    uint32_t c = (uint32_t)(h >= 0x5e2d58d8b3bcdf1aull) + (uint32_t)(h >= 0xbc5ab1b16779be35ull) + (uint32_t)(h >= 0xeb715e1dc1582dc2ull) +
                 (uint32_t)(h >= 0xfb23979734a252f1ull);
    if (c == 4)
        for (int m = 4; m < kPoissonEntries && h >= kPoissonCdf[m]; ++m) ++c;
    return c;
}

__device__ inline uint32_t weight_of(uint32_t row, uint64_t rk, uint32_t i) { return row == 0 ? 1u : poisson1(rk, i); }

// ------------------------------------------------------------------------------------------------ totals
// totals[row] = {N*, n_a*, n_d*}. A label other than 0, 1, 2 cannot be refused without a read-back: every entry of totals becomes
// UINT64_MAX instead (the row's other outputs are then undefined), which the caller of a stream-ordered call can test when it reads them.
__global__ __launch_bounds__(kThreads) void totals_kernel(const uint8_t *labels, uint32_t n, uint64_t seed, uint64_t *totals) {
    const uint32_t row = blockIdx.x;
    const uint64_t rk = row_key(seed, row);
    uint64_t na = 0, nd = 0;
    uint32_t bad = 0;
    for (uint32_t i = threadIdx.x; i < n; i += kThreads) {
        const uint32_t l = labels[i];
        bad |= l > 2u;
        if (l < 2u) {
            const uint64_t c = weight_of(row, rk, i);
            if (l) na += c;
            else nd += c;
        }
    }
    __shared__ uint64_t sa[kThreads], sd[kThreads];
    __shared__ uint32_t sb[kThreads];
    sa[threadIdx.x] = na, sd[threadIdx.x] = nd, sb[threadIdx.x] = bad;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) {
            sa[threadIdx.x] += sa[threadIdx.x + s];
            sd[threadIdx.x] += sd[threadIdx.x + s];
            sb[threadIdx.x] |= sb[threadIdx.x + s];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const bool refuse = sb[0] != 0;
        totals[3 * (uint64_t)row + 0] = refuse ? UINT64_MAX : sa[0] + sd[0];
        totals[3 * (uint64_t)row + 1] = refuse ? UINT64_MAX : sa[0];
        totals[3 * (uint64_t)row + 2] = refuse ? UINT64_MAX : sd[0];
    }
}

// ------------------------------------------------------------------------------------------------ keys and ranked bytes
constexpr uint32_t kKeyUncounted = 0xffffffffu; // after the key of -inf (0xff800000), the last real one

__global__ __launch_bounds__(kThreads) void keys_kernel(const float *scores, const int32_t *status, const uint8_t *labels, uint32_t n, uint32_t *keys, uint32_t *idx) {
    const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= n) return;
    float s = scores[i];
    if (s != s || (status && status[i] != 0)) s = -INFINITY;
    keys[i] = labels[i] < 2u ? pmx::score_rank_key(s) : kKeyUncounted; // (-0.0 and +0.0 are one value)
    idx[i] = i;
}

__global__ __launch_bounds__(kThreads) void ranked_kernel(const uint32_t *keys_sorted, const uint32_t *idx_sorted, const uint8_t *labels, uint32_t n, uint8_t *ranked,
                                                          int64_t *order, uint64_t order_stride) {
    const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
    if (p >= n) return;
    const uint32_t key = keys_sorted[p], i = idx_sorted[p];
    const bool head = p == 0 || keys_sorted[p - 1] != key;
    const bool counted = key != kKeyUncounted;
    ranked[p] = (uint8_t)((labels[i] == 1u ? 1u : 0u) | (head ? 2u : 0u) | (counted ? 4u : 0u));
    if (order && counted && p < order_stride) order[p] = (int64_t)i;
}

// ------------------------------------------------------------------------------------------------ the walk
// The scan's element. sw, sa: weight and active weight of the tie group that is open (since its head); tw, ta: of the list so far.
struct Seg {
    uint64_t sw, sa, tw, ta;
    uint32_t f; // a head lies in the span
};

__device__ inline Seg seg_join(const Seg &l, const Seg &r) {
    Seg o;
    o.f = l.f | r.f;
    o.sw = r.f ? r.sw : l.sw + r.sw;
    o.sa = r.f ? r.sa : l.sa + r.sa;
    o.tw = l.tw + r.tw;
    o.ta = l.ta + r.ta;
    return o;
}

__device__ inline Seg seg_shfl_up(const Seg &v, int d) {
    Seg o;
    o.sw = __shfl_up((unsigned long long)v.sw, d);
    o.sa = __shfl_up((unsigned long long)v.sa, d);
    o.tw = __shfl_up((unsigned long long)v.tw, d);
    o.ta = __shfl_up((unsigned long long)v.ta, d);
    o.f = __shfl_up(v.f, d);
    return o;
}

struct Cuts {
    uint32_t ppm[PMX_ENRICH_MAX_CUTOFFS];
};

struct WalkOut {
    uint64_t *u2;   // [n_cols][rows]
    double *hits;   // [n_cols][rows][n_cut]
    double *expsum; // [n_cols][rows]
};

// What one thread gathers over the walk.
struct Acc {
    uint64_t u2;
    double ex;
};

// The group whose state before the next head (or at the end of the list) is `g` is complete.
__device__ inline void close_group(const Seg &g, Acc &acc, double s_exp, double inv_e1, const uint64_t *cut_k, uint32_t n_cut, uint64_t kmin, uint64_t kmax, double *hits) {
    const uint64_t c = g.sw;
    if (c == 0) return; // (no counted weight: nothing ranks here)
    const uint64_t a = g.sa, d = c - a;
    const uint64_t c_before = g.tw - c, a_before = g.ta - a;
    acc.u2 += d * (2 * a_before + a);
    if (kmin <= g.tw && kmax > c_before)
        for (uint32_t j = 0; j < n_cut; ++j) {
            const uint64_t k = cut_k[j];
            if (k > c_before && k <= g.tw)
                hits[j] = k == g.tw ? (double)(a_before + a) : (double)a_before + (double)a * (double)(k - c_before) / (double)c;
        }
    if (a) acc.ex += (double)a * (exp(s_exp * (double)(c_before + 1)) * expm1(s_exp * (double)c) * inv_e1 / (double)c);
}

__global__ __launch_bounds__(kThreads) void walk_kernel(const uint8_t *ranked_all, const uint32_t *idx_all, uint64_t ranked_stride, uint64_t idx_stride, uint32_t n,
                                                         const uint64_t *totals, uint32_t rows, Cuts cuts, uint32_t n_cut, double alpha, uint64_t seed,
                                                         WalkOut out) {
    const uint32_t col = blockIdx.x, row = blockIdx.y;
    const uint32_t t = threadIdx.x, lane = t % 64, wave = t / 64;
    const uint8_t *ranked = ranked_all + (uint64_t)col * ranked_stride;
    const uint32_t *idx = idx_all + (uint64_t)col * idx_stride;
    const uint64_t rk = row_key(seed, row);
    const uint64_t n_star = totals[3 * (uint64_t)row];
    double *hits = out.hits + ((uint64_t)col * rows + row) * n_cut;

    __shared__ uint64_t cut_k[PMX_ENRICH_MAX_CUTOFFS];
    if (t < n_cut) cut_k[t] = ((uint64_t)cuts.ppm[t] * n_star + 999999ull) / 1000000ull; // (ppm <= 10^6 and N* < 2^36: no overflow)
    __shared__ Seg wave_tot[2][kWaves];
    __shared__ uint64_t red_u2[kThreads];
    __shared__ double red_ex[kThreads];
    __syncthreads();
    uint64_t kmin = UINT64_MAX, kmax = 0;
    for (uint32_t j = 0; j < n_cut; ++j) kmin = min(kmin, cut_k[j]), kmax = max(kmax, cut_k[j]);
    const double s_exp = -alpha / (double)n_star;
    const double inv_e1 = 1.0 / expm1(s_exp);

    Seg carry = {0, 0, 0, 0, 0};
    Acc acc = {0, 0.0};
    const uint32_t n_tiles = (n + kTile - 1) / kTile;
    for (uint32_t tile = 0; tile < n_tiles; ++tile) {
        const uint32_t p0 = tile * kTile + t * kItems;
        uint32_t by[kItems], ix[kItems];
        if (p0 + kItems <= n) { // (both strides are multiples of 16 bytes)
            const uint2 b8 = *reinterpret_cast<const uint2 *>(ranked + p0);
            const uint4 i0 = *reinterpret_cast<const uint4 *>(idx + p0), i1 = *reinterpret_cast<const uint4 *>(idx + p0 + 4);
#pragma unroll
            for (int j = 0; j < 4; ++j) by[j] = (b8.x >> (8 * j)) & 0xffu, by[4 + j] = (b8.y >> (8 * j)) & 0xffu;
            ix[0] = i0.x, ix[1] = i0.y, ix[2] = i0.z, ix[3] = i0.w, ix[4] = i1.x, ix[5] = i1.y, ix[6] = i1.z, ix[7] = i1.w;
        } else {
#pragma unroll
            for (int j = 0; j < kItems; ++j) {
                const bool in = p0 + j < n;
                by[j] = in ? ranked[p0 + j] : 0u; // (past the end: not counted, no head)
                ix[j] = in ? idx[p0 + j] : 0u;
            }
        }
        uint32_t w[kItems];
        Seg mine = {0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            w[j] = (by[j] & 4u) ? weight_of(row, rk, ix[j]) : 0u;
            const Seg e = {w[j], (by[j] & 1u) ? w[j] : 0u, w[j], (by[j] & 1u) ? w[j] : 0u, (by[j] >> 1) & 1u};
            mine = seg_join(mine, e);
        }
        // inclusive scan of the threads' spans inside the wavefront, then the wavefronts' totals through LDS
        Seg inc = mine;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const Seg o = seg_shfl_up(inc, d);
            if ((int)lane >= d) inc = seg_join(o, inc);
        }
        Seg (&wt)[kWaves] = wave_tot[tile & 1];
        if (lane == 63) wt[wave] = inc;
        __syncthreads(); // (two buffers: the totals of tile - 1 may still be read by a wavefront that is behind)
        Seg before = seg_shfl_up(inc, 1); // the wavefront's threads ahead of this one
        if (lane == 0) before = Seg{0, 0, 0, 0, 0};
        Seg st = carry; // -> everything ahead of this thread's first position: the tiles before, the wavefronts before, `before`
        for (uint32_t v = 0; v < wave; ++v) st = seg_join(st, wt[v]);
        st = seg_join(st, before);
        for (uint32_t v = 0; v < kWaves; ++v) carry = seg_join(carry, wt[v]);
#pragma unroll
        for (int j = 0; j < kItems; ++j) {
            if (by[j] & 2u) close_group(st, acc, s_exp, inv_e1, cut_k, n_cut, kmin, kmax, hits);
            const Seg e = {w[j], (by[j] & 1u) ? w[j] : 0u, w[j], (by[j] & 1u) ? w[j] : 0u, (by[j] >> 1) & 1u};
            st = seg_join(st, e);
        }
    }
    if (t == 0) close_group(carry, acc, s_exp, inv_e1, cut_k, n_cut, kmin, kmax, hits);
    red_u2[t] = acc.u2, red_ex[t] = acc.ex;
    __syncthreads();
    for (int s = kThreads / 2; s > 0; s >>= 1) {
        if ((int)t < s) red_u2[t] += red_u2[t + s], red_ex[t] += red_ex[t + s];
        __syncthreads();
    }
    if (t == 0) {
        out.u2[(uint64_t)col * rows + row] = red_u2[0];
        out.expsum[(uint64_t)col * rows + row] = red_ex[0];
    }
}

// ------------------------------------------------------------------------------------------------ host
// Work buffers kept from call to call, one set per device (DevBuf: grow-only, a wait for the call's stream before a reallocation). The
// call does not wait for its stream, so a call on another stream starts behind the event the call before it left.
struct EnrichWork {
    std::mutex mu;
    pmx::DevBuf keys_in, keys_out, idx_in, idx, ranked, sort;
    hipEvent_t done = nullptr;
    hipStream_t last = nullptr;
    bool pending = false;
    // pmx_set_profiling(1): call start | totals done | per column: sorted, ranked bytes written | walk done (pmx_enrichment_times)
    std::vector<hipEvent_t> ev;
    int ev_cols = 0; // columns of the last profiled call; 0: none
};
constexpr int kMaxDevices = 64;
EnrichWork g_work[kMaxDevices];

uint64_t round_up(uint64_t x, uint64_t m) { return (x + m - 1) / m * m; }

} // namespace

extern "C" int pmx_enrichment(const float *scores_dev, uint64_t col_stride, int n_cols, uint64_t n, const int32_t *status_dev, const uint8_t *labels_dev,
                              const uint32_t *cut_ppm, int n_cut, double alpha, int n_boot, uint64_t seed, uint64_t *totals_dev, uint64_t *u2_dev, double *hits_dev,
                              double *expsum_dev, int64_t *order_dev, uint64_t order_stride, int device, void *stream_) {
    if (!scores_dev || !labels_dev || !totals_dev || !u2_dev || !expsum_dev || (n_cut > 0 && (!cut_ppm || !hits_dev)))
        return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: null argument");
    if (n_cols < 1 || n_cols > PMX_ENRICH_MAX_COLUMNS) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: 1 to %d columns, not %d", PMX_ENRICH_MAX_COLUMNS, n_cols);
    if (n < 1 || n > 0x7fffffffull) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: 1 to 2^31 - 1 ligands");
    if (col_stride < n) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: col_stride below n");
    if (n_cut < 0 || n_cut > PMX_ENRICH_MAX_CUTOFFS) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: 0 to %d cutoffs, not %d", PMX_ENRICH_MAX_CUTOFFS, n_cut);
    for (int j = 0; j < n_cut; ++j)
        if (cut_ppm[j] < 1 || cut_ppm[j] > 1000000u) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: cutoff %d is %u ppm (1 to 1000000)", j, cut_ppm[j]);
    if (!(alpha > 0.0) || !std::isfinite(alpha)) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: alpha must be positive and finite");
    if (n_boot < 0 || n_boot > PMX_ENRICH_MAX_BOOTSTRAP) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: 0 to %d resamples, not %d", PMX_ENRICH_MAX_BOOTSTRAP, n_boot);
    if (device < 0 || device >= kMaxDevices) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment: device index out of range");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    PMX_HIPCHECK(hipSetDevice(device));
    const uint32_t n32 = (uint32_t)n, rows = 1u + (uint32_t)n_boot;
    const uint64_t idx_stride = round_up(n, 4), ranked_stride = round_up(n, 16); // rows of the ranked buffers start on 16-byte boundaries

    EnrichWork &w = g_work[device];
    std::lock_guard<std::mutex> lock(w.mu);
    if (!w.done) PMX_HIPCHECK(hipEventCreateWithFlags(&w.done, hipEventDisableTiming));
    if (w.pending && w.last != stream) PMX_HIPCHECK(hipStreamWaitEvent(stream, w.done, 0));
    size_t sort_need = 0;
    PMX_HIPCHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_need, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, (int)n, 0,
                                                    32, stream));
    // (a buffer that grows is freed after a wait for this stream, which by now runs behind the call before: nothing uses it any more)
    hipError_t e = w.keys_in.grow(n * 4, stream);
    if (e == hipSuccess) e = w.keys_out.grow(n * 4, stream);
    if (e == hipSuccess) e = w.idx_in.grow(n * 4, stream);
    if (e == hipSuccess) e = w.idx.grow((uint64_t)n_cols * idx_stride * 4, stream);
    if (e == hipSuccess) e = w.ranked.grow((uint64_t)n_cols * ranked_stride, stream);
    if (e == hipSuccess) e = w.sort.grow(sort_need ? sort_need : 16, stream);
    PMX_HIPCHECK(e);
    Cuts cuts = {}; // (the cutoffs travel as a kernel argument: no copy from the caller's memory to order)
    for (int j = 0; j < n_cut; ++j) cuts.ppm[j] = cut_ppm[j];
    // a cutoff that no group straddles (N* = 0) keeps 0
    if (n_cut) PMX_HIPCHECK(hipMemsetAsync(hits_dev, 0, (size_t)n_cols * rows * (size_t)n_cut * sizeof(double), stream));

    const bool timed = pmx_profiling() != 0;
    w.ev_cols = 0;
    while (timed && w.ev.size() < 3 + 2 * (size_t)n_cols) {
        hipEvent_t ev = nullptr;
        PMX_HIPCHECK(hipEventCreate(&ev));
        w.ev.push_back(ev);
    }
    const unsigned blocks = (unsigned)((n + kThreads - 1) / kThreads);
    if (timed) PMX_HIPCHECK(hipEventRecord(w.ev[0], stream));
    totals_kernel<<<dim3(rows), dim3(kThreads), 0, stream>>>(labels_dev, n32, seed, totals_dev);
    if (timed) PMX_HIPCHECK(hipEventRecord(w.ev[1], stream));
    for (int c = 0; c < n_cols; ++c) {
        uint32_t *idx_c = w.idx.as<uint32_t>() + (uint64_t)c * idx_stride;
        keys_kernel<<<dim3(blocks), dim3(kThreads), 0, stream>>>(scores_dev + (uint64_t)c * col_stride, status_dev, labels_dev, n32, w.keys_in.as<uint32_t>(),
                                                                 w.idx_in.as<uint32_t>());
        size_t sort_bytes = w.sort.bytes;
        PMX_HIPCHECK(hipcub::DeviceRadixSort::SortPairs(w.sort.ptr, sort_bytes, w.keys_in.as<uint32_t>(), w.keys_out.as<uint32_t>(), w.idx_in.as<uint32_t>(), idx_c, (int)n, 0, 32,
                                                        stream));
        if (timed) PMX_HIPCHECK(hipEventRecord(w.ev[2 + 2 * c], stream));
        ranked_kernel<<<dim3(blocks), dim3(kThreads), 0, stream>>>(w.keys_out.as<uint32_t>(), idx_c, labels_dev, n32, w.ranked.as<uint8_t>() + (uint64_t)c * ranked_stride,
                                                                   order_dev ? order_dev + (uint64_t)c * order_stride : nullptr, order_stride);
        if (timed) PMX_HIPCHECK(hipEventRecord(w.ev[3 + 2 * c], stream));
    }
    WalkOut out = {u2_dev, hits_dev, expsum_dev};
    walk_kernel<<<dim3((unsigned)n_cols, rows), dim3(kThreads), 0, stream>>>(w.ranked.as<uint8_t>(), w.idx.as<uint32_t>(), ranked_stride, idx_stride, n32, totals_dev, rows,
                                                                            cuts, (uint32_t)n_cut, alpha, seed, out);
    PMX_HIPCHECK(hipGetLastError());
    if (timed) {
        PMX_HIPCHECK(hipEventRecord(w.ev[2 + 2 * n_cols], stream));
        w.ev_cols = n_cols;
    }
    PMX_HIPCHECK(hipEventRecord(w.done, stream));
    w.last = stream;
    w.pending = true;
    return PMX_OK;
}

extern "C" int pmx_enrichment_times(int device, double ms_out[4]) {
    if (!ms_out || device < 0 || device >= kMaxDevices) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment_times: bad argument");
    EnrichWork &w = g_work[device];
    std::lock_guard<std::mutex> lock(w.mu);
    if (!w.ev_cols) return pmx_fail(PMX_ERR_INVALID, "pmx_enrichment_times: no profiled pmx_enrichment on this device (pmx_set_profiling(1) first)");
    PMX_HIPCHECK(hipSetDevice(device));
    PMX_HIPCHECK(hipEventSynchronize(w.ev[2 + 2 * w.ev_cols]));
    auto between = [&](int a, int b, double &sum) {
        float ms = 0.f;
        const hipError_t e = hipEventElapsedTime(&ms, w.ev[a], w.ev[b]);
        sum += ms;
        return e;
    };
    double totals = 0, sort = 0, ranked = 0, walk = 0;
    PMX_HIPCHECK(between(0, 1, totals));
    for (int c = 0; c < w.ev_cols; ++c) {
        PMX_HIPCHECK(between(1 + 2 * c, 2 + 2 * c, sort));
        PMX_HIPCHECK(between(2 + 2 * c, 3 + 2 * c, ranked));
    }
    PMX_HIPCHECK(between(1 + 2 * w.ev_cols, 2 + 2 * w.ev_cols, walk));
    ms_out[0] = totals, ms_out[1] = sort, ms_out[2] = ranked, ms_out[3] = walk;
    return PMX_OK;
}

// pmx_release_workspaces: the unit's buffers of `device` (the device is current and idle).
int pmx_enrich_release(int device) {
    if (device < 0 || device >= kMaxDevices) return PMX_OK;
    EnrichWork &w = g_work[device];
    std::lock_guard<std::mutex> lock(w.mu); // a call that is enqueuing finishes first
    for (pmx::DevBuf *b : {&w.keys_in, &w.keys_out, &w.idx_in, &w.idx, &w.ranked, &w.sort}) b->release();
    if (w.done) (void)hipEventDestroy(w.done);
    for (hipEvent_t ev : w.ev) (void)hipEventDestroy(ev);
    w.ev.clear();
    w.done = nullptr, w.last = nullptr, w.pending = false, w.ev_cols = 0;
    return PMX_OK;
}
