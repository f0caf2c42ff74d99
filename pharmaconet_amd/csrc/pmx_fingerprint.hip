// pmx_fingerprint.hip - what is done with the interaction fingerprints pmx_hotspots writes (include/pmx.h), on gfx950: the Tanimoto
// similarity of two lists of fingerprints, and sphere exclusion in row order (leaders). A fingerprint is PMX_FINGERPRINT_WORDS 64-bit
// words, a bit per model node.
//
// tanimoto_kernel - a thread keeps one fingerprint of b in registers and walks kRowsPerBlock fingerprints of a, whose words every lane
// of the wavefront reads from one address: the 256 threads of a block write 256 consecutive floats of a row of the block at a time.
//
// leaders_kernel - one work-group; the leaders' fingerprints live in LDS in the order they were made, which is row order. Rows are taken
// kBlock at a time, a row per thread:
//   join      every row of the block against the leaders made before the block, in order, until one is similar enough
//   resolve   the rows that joined none, among themselves: the first of them becomes a leader (while there is room), the later ones of
//             them are compared with it and join it if similar enough; again until none is left. A row reaches a leader made in its own
//             block only after every earlier leader has refused it, so it joins the first leader that takes it - the definition.
// Integer arithmetic and one float32 division per comparison: the result does not depend on kBlock.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "pmx.h"
#include "pmx_device.h"

namespace {
constexpr int kW = PMX_FINGERPRINT_WORDS;
static_assert(kW == 4, "a fingerprint is four words");

struct Fp {
    unsigned long long w[kW];
};

__device__ __forceinline__ Fp load_fp(const uint64_t *p, size_t i) {
    Fp f;
#pragma unroll
    for (int j = 0; j < kW; ++j) f.w[j] = p[i * kW + j];
    return f;
}

// popcount(x & y) / popcount(x | y) as one float32 division; 1 when both are empty.
__device__ __forceinline__ float tanimoto(const Fp &x, const Fp &y) {
    int both = 0, any = 0;
#pragma unroll
    for (int j = 0; j < kW; ++j) {
        both += __popcll(x.w[j] & y.w[j]);
        any += __popcll(x.w[j] | y.w[j]);
    }
    return any == 0 ? 1.0f : (float)both / (float)any;
}

constexpr int kRowsPerBlock = 32;

__global__ __launch_bounds__(256) void tanimoto_kernel(const uint64_t *a, uint32_t na, const uint64_t *b, uint32_t nb, float *out) {
    const uint32_t j = blockIdx.x * 256u + threadIdx.x;
    const uint32_t i0 = blockIdx.y * (uint32_t)kRowsPerBlock;
    if (j >= nb) return;
    const Fp y = load_fp(b, j);
    const uint32_t i1 = min(na, i0 + (uint32_t)kRowsPerBlock);
    for (uint32_t i = i0; i < i1; ++i) out[(size_t)i * nb + j] = tanimoto(load_fp(a, i), y);
}

constexpr int kBlock = 1024;
constexpr uint32_t kNone = 0xFFFFFFFFu;

__global__ __launch_bounds__(kBlock) void leaders_kernel(const uint64_t *fp, uint32_t n, float threshold, uint32_t max_leaders, uint32_t *leader_of,
                                                          uint32_t *leaders, uint32_t *n_leaders) {
    __shared__ unsigned long long lfp[PMX_MAX_LEADERS][kW]; // the leaders' fingerprints
    __shared__ uint32_t lrow[PMX_MAX_LEADERS];              // and rows
    __shared__ uint32_t first;                              // resolve: the first thread whose row has joined none
    const uint32_t t = threadIdx.x;
    uint32_t nl = 0; // leaders so far (the same in every thread)
    for (uint32_t r0 = 0; r0 < n; r0 += (uint32_t)kBlock) {
        const uint32_t row = r0 + t;
        const bool have = row < n;
        Fp x{};
        if (have) x = load_fp(fp, row);
        // ---- join
        bool open = have; // the row has joined no leader yet
        uint32_t mine = kNone;
        for (uint32_t k = 0; k < nl && open; ++k) {
            Fp y;
#pragma unroll
            for (int j = 0; j < kW; ++j) y.w[j] = lfp[k][j];
            if (tanimoto(x, y) >= threshold) {
                mine = lrow[k];
                open = false;
            }
        }
        // ---- resolve
        for (;;) {
            if (t == 0) first = kNone;
            __syncthreads();
            if (open) atomicMin(&first, t);
            __syncthreads();
            const uint32_t f = first;
            __syncthreads(); // (everybody has read `first` before thread 0 resets it)
            if (f == kNone || nl >= max_leaders) break;
            if (t == f) {
#pragma unroll
                for (int j = 0; j < kW; ++j) lfp[nl][j] = x.w[j];
                lrow[nl] = row;
                leaders[nl] = row;
                mine = row;
                open = false;
            }
            __syncthreads();
            if (open) { // (t > f: f was the first)
                Fp y;
#pragma unroll
                for (int j = 0; j < kW; ++j) y.w[j] = lfp[nl][j];
                if (tanimoto(x, y) >= threshold) {
                    mine = r0 + f;
                    open = false;
                }
            }
            ++nl;
        }
        if (have) leader_of[row] = mine; // (still open: no room for another leader)
    }
    if (t == 0) *n_leaders = nl;
}

} // namespace

extern "C" int pmx_fingerprint_tanimoto(const uint64_t *a_dev, uint32_t na, const uint64_t *b_dev, uint32_t nb, float *out_dev, int device, void *stream_) {
    if (na > PMX_EXPLAIN_MAX || nb > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_tanimoto: more than 65536 fingerprints on a side");
    if (na == 0 || nb == 0) return PMX_OK;
    if (!a_dev || !b_dev || !out_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_tanimoto: null argument");
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_fingerprint_tanimoto: hipSetDevice failed");
    const dim3 grid((nb + 255u) / 256u, (na + (uint32_t)kRowsPerBlock - 1u) / (uint32_t)kRowsPerBlock);
    tanimoto_kernel<<<grid, dim3(256), 0, static_cast<hipStream_t>(stream_)>>>(a_dev, na, b_dev, nb, out_dev);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}

extern "C" int pmx_fingerprint_leaders(const uint64_t *fp_dev, uint32_t n, float threshold, uint32_t max_leaders, uint32_t *leader_of_dev, uint32_t *leaders_dev,
                                       uint32_t *n_leaders_dev, int device, void *stream_) {
    if (!(threshold > 0.0f && threshold <= 1.0f)) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_leaders: the threshold is not in (0, 1]");
    if (max_leaders == 0 || max_leaders > PMX_MAX_LEADERS) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_leaders: max_leaders is not in 1 .. 2048");
    if (n > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_leaders: more than 65536 fingerprints");
    if (!n_leaders_dev || (n && (!fp_dev || !leader_of_dev || !leaders_dev))) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_leaders: null argument");
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_fingerprint_leaders: hipSetDevice failed");
    leaders_kernel<<<dim3(1), dim3(kBlock), 0, static_cast<hipStream_t>(stream_)>>>(fp_dev, n, threshold, max_leaders, leader_of_dev, leaders_dev, n_leaders_dev);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
