// pmx_device.h - device-side layouts shared by the kernels of libpmx (gfx950 only), and what the host halves of the .hip units share: the
// check of a HIP call (PMX_HIPCHECK), the functions one unit offers the others, the dispatch on the kernels' lane count (with_lanes) and
// the owner of a cached device buffer (DevBuf).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "pmx.h"
#include "pmx_error.h"

// Host: returns from the calling function with the thread's message set when a HIP call fails.
#define PMX_HIPCHECK(expr)                                                                                         \
    do {                                                                                                           \
        hipError_t e_ = (expr);                                                                                    \
        if (e_ != hipSuccess)                                                                                      \
            return pmx_fail(e_ == hipErrorOutOfMemory ? PMX_ERR_OOM : PMX_ERR_HIP, "%s failed: %s (%s:%d)", #expr, \
                            hipGetErrorString(e_), __FILE__, __LINE__);                                            \
    } while (0)

// Host: what the units of libpmx.so call in one another, outside include/pmx.h. (What stands behind a model or library handle: pmx_handles.h.)
int pmx_topk_release(int device);               // pmx_topk.hip, pmx_pack_device.hip, pmx_select.hip: free the unit's cached buffers
int pmx_pack_release(int device);               //   of `device` (pmx_release_workspaces)
int pmx_select_release(int device);
int pmx_enrich_release(int device);             // pmx_enrich.hip
int pmx_profiling();                            // pmx_api.hip: what pmx_set_profiling set

namespace pmx {

// Device copy of one pharmacophore model. `edge[m * Nm + n]` = {mean, s, T, std}:
//   s = sqrt(0.5 * log2(e)) / std     so that exp(-0.5 z^2) = exp2(-(|d - mean| * s)^2)
//   T = the largest float with  fl(T / std) < 2  (fl = float32 division, round to nearest even),
//       so `|d - mean| <= T` is bit-for-bit the reference's `abs((d - mean) / std) < 2.0`
//       (src/pmnet/scoring/match_utils.py:55-57) without a division in the inner loop.
struct DevModel {
    int32_t Nm, K;
    int32_t symmetric;        // edge[m][n] == edge[n][m] bit for bit (distances are; checked when the model is created)
    int32_t pad_;
    const float4 *edge;       // [Nm * Nm]
    const uint8_t *node_type; // [PMX_MAX_MODEL_NODES]
    const uint64_t *tclus;    // [128][2] ligand cluster type mask -> model clusters sharing a type (graph_match.py:130-134), 128 bits
    const float2 *cpair;      // [K * K] {float32(|center_a - center_b|), float32(size_a + size_b)}  (graph_match.py:263-265)
    const float2 *cwin;       // [K * K] {lo, hi}: the hull of the 2-sigma pass windows of every node pair (m in a, n in b) - a ligand
                              // node pair at a distance outside it fails the majority test of match_utils.py:55-61 against every
                              // pair of node subsets of the two clusters (exact float ends, as `T` above; {+inf, -inf}: no window)
};

struct DevLibrary {
    uint64_t n;
    const uint64_t *offsets;
    const uint8_t *data;
};

struct Weights {
    float w[PMX_NUM_TYPES];
};

__host__ __device__ inline uint64_t round16(uint64_t x) { return (x + 15) & ~uint64_t(15); }

// Rank key of a real score (not a NaN), the one definition for every unit that ranks (pmx_topk.hip, pmx_enrich.hip): an ascending key
// is a descending score, equal scores have equal keys. -0.0 and +0.0 are one value, so the zero is made +0.0 before its bits are read
// (the units are built with -fno-fast-math: the comparison stays). +inf -> 0x007fffff, +-0.0 -> 0x7fffffff, -inf -> 0xff800000, the
// largest key of a real score; the keys above it are the callers' (NaN, padding, uncounted).
__host__ __device__ inline uint32_t score_rank_key(float s) {
    if (s == 0.0f) s = 0.0f;
    uint32_t u = __builtin_bit_cast(uint32_t, s);
    u = (u >> 31) ? ~u : (u | 0x80000000u); // ascending with the float
    return ~u;
}

// A ligand record of the packed library (pharmaconet_amd/library.py).
struct Record {
    int n, C, ncl;
    const uint8_t *typemask;
    const uint8_t *cluster_end;
    const float *xyz; // [n][3][C]
};

__device__ inline Record parse_record(const uint8_t *rec) {
    Record r;
    const uint16_t *h = reinterpret_cast<const uint16_t *>(rec);
    r.n = h[0];
    r.C = h[1];
    r.ncl = h[2];
    r.typemask = rec + 8;
    r.cluster_end = rec + 8 + r.n;
    uint32_t off = (8u + uint32_t(r.n) + uint32_t(r.ncl) + 3u) & ~3u;
    r.xyz = reinterpret_cast<const float *>(rec + off);
    return r;
}

__device__ inline bool record_supported(const Record &r) {
    return r.C >= 1 && r.C <= PMX_MAX_CONFORMERS && r.n <= PMX_MAX_LIGAND_NODES && r.ncl <= PMX_MAX_LIGAND_CLUSTERS;
}

// Host: f(std::integral_constant<int, G>{}) for a conformer lane count the kernels are built for (1, 2, 4, ..., 64); false for any other G.
template <class F>
inline bool with_lanes(int G, F &&f) {
    switch (G) {
    case 1: f(std::integral_constant<int, 1>{}); return true;
    case 2: f(std::integral_constant<int, 2>{}); return true;
    case 4: f(std::integral_constant<int, 4>{}); return true;
    case 8: f(std::integral_constant<int, 8>{}); return true;
    case 16: f(std::integral_constant<int, 16>{}); return true;
    case 32: f(std::integral_constant<int, 32>{}); return true;
    case 64: f(std::integral_constant<int, 64>{}); return true;
    default: return false;
    }
}

// Host: a device buffer that is kept from call to call and has this one owner. It only ever grows. Work queued on `stream` may still
// use the old buffer, so a reallocation waits for that stream first. min_bytes: the buffer is a cache (the table arena) - a smaller
// one is slower, never wrong: the size asked for is halved on out-of-memory, down to min_bytes, and `bytes` says what it got.
// No destructor: buffers are freed by release(), while the HIP runtime is alive and the right device is current.
struct DevBuf {
    void *ptr = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    template <class T>
    T *as() const { return static_cast<T *>(ptr); }
    hipError_t grow(size_t want, hipStream_t stream, size_t min_bytes = 0) {
        if (bytes >= want) return hipSuccess;
        if (ptr) {
            const hipError_t e = hipStreamSynchronize(stream);
            if (e != hipSuccess) return e;
            release();
        }
        for (;;) {
            const hipError_t e = hipMalloc(&ptr, want);
            if (e == hipSuccess) break;
            (void)hipGetLastError();
            ptr = nullptr;
            if (e != hipErrorOutOfMemory || min_bytes == 0 || want / 2 < min_bytes) return e;
            want /= 2;
        }
        bytes = want;
        return hipSuccess;
    }
    void release() {
        if (ptr) (void)hipFree(ptr);
        ptr = nullptr;
        bytes = 0;
    }
};

} // namespace pmx
