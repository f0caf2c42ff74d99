// pmx_ligand_fp.hip - a ligand described by its own pharmacophore, on gfx950: pmx_library_fingerprints writes a 252-bit two-point
// fingerprint (type pair x distance bin) and a type census per ligand of a resident library, pmx_fingerprint_search compares up to 64 query
// fingerprints with a list of any length. The definitions are the comments of include/pmx.h; tests/ligand_fp_ref.py restates them in NumPy.
//
// ligand_fp_kernel - one wavefront per ligand, kWaves per block, nothing shared between the waves of a block (no LDS array, no barrier). The
// record stores xyz[n][3][C] with the conformer index fastest, so the 64 lanes are S = 64 / G slots of G conformer lanes (G the power of
// two that holds the conformers asked for): lane (s, c) reads conformer c, and the G lanes of a slot read contiguous floats.
//   rows      u runs over the nodes, the same in every lane; the row's partners v = u + 1 + s, + S, ... take the slots, so a record of 64
//             nodes walks its 2016 pairs in 63 rows of one to 63 / S + 1 trips. The u side of a row (its position, its type mask) is read
//             once per row.
//   trip      d2 in float32 as the header gives it, bin = the number of edges it reaches, and the partner's 7-bit type mask spread to
//             bit 9 b of a 64-bit word and shifted by bin: bit 9 b + bin says "a partner of type b in this bin". Lane v holds node v's
//             spread mask (the census has loaded the masks, a lane per node), a trip fetches its partner's with two __shfl. A row ORs
//             its trips.
//   set       m[a], a = 0..6, one 64-bit word per type in the lane's registers: at the end of row u the row's word is ORed into m[a] for
//             every type a of u's mask - u is the same in every lane, so which m[a] is a scalar decision and no register is indexed by a
//             lane's value. m[a] bit 9 b + bin is the unordered type pair {a, b} in that bin.
//   gather    m[0..6] ORed across the 64 lanes (wave_or: DPP moves) into scalars; the 28 type pairs (lo, hi) - nine bits each, bits
//             9 hi .. of m[lo] or bits 9 lo .. of m[hi] - are placed at bit 9 p of the 256 by unrolled scalar code.
// OR is order-free: the bits do not depend on G, S or the order of the rows.
//
// The set is kept in registers. The other layout that was built - a per-wave 256-bit set in LDS and one atomicOr per (type pair, bin) of
// every trip - was measured next to it and was the slower one over all conformers, by a tenth at 8 conformers and 2.5 times at 64; the
// numbers are in DESIGN.md section 3.
//
// search_kernel - one thread per library fingerprint, read once and compared with every query; the queries are
// read through addresses that are the same in every lane. Thread i writes out[q][i] for q = 0 .. nq - 1 (256 consecutive floats of a
// row per block at a time) and the maximum over q.
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_handles.h"

namespace {
using pmx::parse_record;
using pmx::Record;
using pmx::record_supported;

constexpr int kW = PMX_FINGERPRINT_WORDS;
static_assert(kW == 4, "a fingerprint is four words");
static_assert(PMX_LFP_BINS == 9 && PMX_NUM_TYPES == 7 && 28 * PMX_LFP_BINS <= 64 * kW, "28 type pairs of 9 bins fit 256 bits");
static_assert(PMX_MAX_LIGAND_NODES <= 64, "the census takes a lane per node");

constexpr int kWaves = 4;
constexpr unsigned long long kSpreadMul = 0x0001010101010101ull;  // copy k of a 7-bit mask at bit 8 k ...
constexpr unsigned long long kSpreadMask = 0x0040201008040201ull; // ... of which bit b of copy b is bit 9 b

// The number of entries of E2 = {4, 9, 16, 25, 36, 56.25, 81, 144} that d2 reaches; 0 for a NaN.
__device__ __forceinline__ int distance_bin(float d2) {
    return (int)(d2 >= 4.0f) + (int)(d2 >= 9.0f) + (int)(d2 >= 16.0f) + (int)(d2 >= 25.0f) + (int)(d2 >= 36.0f) + (int)(d2 >= 56.25f) + (int)(d2 >= 81.0f) +
           (int)(d2 >= 144.0f);
}

// OR over the 64 lanes, as a scalar. Data-parallel-primitive moves, no LDS traffic: inside a row of 16 lanes a butterfly (the quad's pairs,
// the quad's halves, the half row mirrored, the row mirrored) leaves the row's OR in each of its lanes; lane 15 of a row is then broadcast
// into the next row (rows 1 and 3), lane 31 into rows 2 and 3, and lane 63 holds all four. A lane a move does not write takes 0.
__device__ __forceinline__ uint32_t wave_or(uint32_t x) {
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0xB1, 0xF, 0xF, true);   // quad_perm [1, 0, 3, 2]
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x4E, 0xF, 0xF, true);   // quad_perm [2, 3, 0, 1]
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x141, 0xF, 0xF, true);  // row_half_mirror
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x140, 0xF, 0xF, true);  // row_mirror
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x142, 0xA, 0xF, false); // row_bcast:15 into rows 1 and 3
    x |= (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x143, 0xC, 0xF, false); // row_bcast:31 into rows 2 and 3
    return (uint32_t)__builtin_amdgcn_readlane((int)x, 63);
}

__global__ __launch_bounds__(64 * kWaves) void ligand_fp_kernel(const uint64_t *__restrict__ lib_offsets, const uint8_t *__restrict__ lib_data, uint64_t first, uint64_t count,
                                                                const int32_t *__restrict__ conformer, uint64_t *__restrict__ fingerprint, uint8_t *__restrict__ type_count,
                                                                int32_t *__restrict__ status) {
    // (everything a wavefront decides by is made a scalar: its ligand, the record's header, the conformer asked for)
    const uint64_t r = (uint64_t)blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (r >= count) return;
    const int lane = (int)(threadIdx.x % 64);
    const uint8_t *rec_bytes = lib_data + lib_offsets[first + r];
    const Record rec = parse_record(rec_bytes);
    const bool supported = __builtin_amdgcn_readfirstlane((int)record_supported(rec)) != 0;
    const int n = supported ? __builtin_amdgcn_readfirstlane(rec.n) : 0, C = __builtin_amdgcn_readfirstlane(rec.C);
    const int sel = conformer ? conformer[r] : -1;
    const bool key_ok = sel >= -1 && sel < C;

    // ---- census: a lane per node
    const uint32_t tm_lane = lane < n ? (uint32_t)rec.typemask[lane] & 0x7Fu : 0u;
    if (type_count) {
        uint32_t mine = 0;
#pragma unroll
        for (int t = 0; t < PMX_NUM_TYPES; ++t) {
            const uint32_t c = (uint32_t)__popcll(__ballot((tm_lane >> t) & 1u));
            if (lane == t) mine = c;
        }
        if (lane == 7) mine = (uint32_t)n;
        if (lane < 8) type_count[r * 8 + lane] = (uint8_t)mine;
    }
    if (status && lane == 0) status[r] = !supported ? PMX_LIGAND_UNSUPPORTED : (key_ok ? PMX_LIGAND_OK : PMX_LIGAND_KEY_INVALID);
    if (!supported || !key_ok || n < 2) {
        if (lane < kW) fingerprint[r * kW + lane] = 0ull;
        return;
    }

    // ---- lanes: S slots of G conformer lanes
    const int c0 = sel >= 0 ? sel : 0, nc = sel >= 0 ? 1 : C;
    int lg = 0;
    while ((1 << lg) < nc) ++lg;
    const int G = 1 << lg, S = 64 >> lg;
    const int slot = lane >> lg, cl = lane & (G - 1);
    const bool c_on = cl < nc;
    // positions are read at 32-bit byte offsets from the record's start: float (u, k, c) of xyz[n][3][C] lies at xyz_at + 4 ((3 u + k) C + c)
    const uint32_t xyz_at = __builtin_amdgcn_readfirstlane((uint32_t)(reinterpret_cast<const uint8_t *>(rec.xyz) - rec_bytes));
    const uint32_t row_bytes = 12u * (uint32_t)C, k_bytes = 4u * (uint32_t)C, at_c = xyz_at + 4u * (uint32_t)(c_on ? c0 + cl : c0);
    const uint32_t at_slot = (uint32_t)slot * row_bytes + at_c;
    const auto coord = [rec_bytes](uint32_t at) { return *reinterpret_cast<const float *>(rec_bytes + at); };
    // node `lane`'s type mask, each type b at bit 9 b: a trip fetches its partner's from lane v
    const unsigned long long spread = ((unsigned long long)tm_lane * kSpreadMul) & kSpreadMask;
    const int spread_lo = (int)(uint32_t)spread, spread_hi = (int)(uint32_t)(spread >> 32);

    unsigned long long m[PMX_NUM_TYPES] = {0ull, 0ull, 0ull, 0ull, 0ull, 0ull, 0ull};
    for (int u = 0; u + 1 < n; ++u) {
        const uint32_t tmu = __builtin_amdgcn_readfirstlane((uint32_t)rec.typemask[u] & 0x7Fu); // (0: the row leaves nothing)
        const uint32_t at_u = (uint32_t)u * row_bytes + at_c;
        const float xu = coord(at_u), yu = coord(at_u + k_bytes), zu = coord(at_u + 2u * k_bytes);
        unsigned long long row = 0ull;
        for (int v0 = u + 1; v0 < n; v0 += S) { // (as many trips in every lane: the shuffles below see all 64)
            const int v = v0 + slot;
            const bool on = c_on && v < n;
            const int src = on ? v : lane;
            const unsigned long long partner = (unsigned long long)(uint32_t)__shfl(spread_lo, src) | ((unsigned long long)(uint32_t)__shfl(spread_hi, src) << 32);
            if (on) {
                const uint32_t at_v = (uint32_t)v0 * row_bytes + at_slot;
                const float dx = xu - coord(at_v), dy = yu - coord(at_v + k_bytes), dz = zu - coord(at_v + 2u * k_bytes);
                const float d2 = (dx * dx + dy * dy) + dz * dz;
                row |= partner << distance_bin(d2);
            }
        }
#pragma unroll
        for (int a = 0; a < PMX_NUM_TYPES; ++a) m[a] |= row & (0ull - (unsigned long long)((tmu >> a) & 1u)); // (a scalar mask: no branch, no select)
    }

    // ---- gather: OR across the lanes into scalars; the 28 type pairs are placed by scalar code
    unsigned long long all[PMX_NUM_TYPES];
#pragma unroll
    for (int a = 0; a < PMX_NUM_TYPES; ++a) all[a] = (unsigned long long)wave_or((uint32_t)m[a]) | ((unsigned long long)wave_or((uint32_t)(m[a] >> 32)) << 32);
    unsigned long long word[kW + 1] = {0ull, 0ull, 0ull, 0ull, 0ull};
#pragma unroll
    for (int lo = 0; lo < PMX_NUM_TYPES; ++lo) {
#pragma unroll
        for (int hi = lo; hi < PMX_NUM_TYPES; ++hi) {
            const int j = (lo * (15 - lo) / 2 + (hi - lo)) * PMX_LFP_BINS; // the pair's first bit
            const unsigned long long nine = ((all[lo] >> (9 * hi)) | (all[hi] >> (9 * lo))) & 0x1FFull;
            word[j / 64] |= nine << (j % 64);
            if (j % 64 > 64 - PMX_LFP_BINS) word[j / 64 + 1] |= nine >> (64 - j % 64);
        }
    }
    if (lane < kW) fingerprint[r * kW + lane] = lane == 0 ? word[0] : lane == 1 ? word[1] : lane == 2 ? word[2] : word[3];
}

__global__ __launch_bounds__(256) void search_kernel(const uint64_t *__restrict__ query, uint32_t nq, const uint64_t *__restrict__ fp, uint64_t n, float *__restrict__ out,
                                                     uint64_t out_stride, float *__restrict__ fused) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    unsigned long long x[kW];
#pragma unroll
    for (int j = 0; j < kW; ++j) x[j] = fp[i * kW + j];
    float best = 0.0f;
    for (uint32_t q = 0; q < nq; ++q) {
        int both = 0, any = 0;
#pragma unroll
        for (int j = 0; j < kW; ++j) {
            const unsigned long long y = query[(size_t)q * kW + j];
            both += __popcll(x[j] & y);
            any += __popcll(x[j] | y);
        }
        const float sim = any == 0 ? 1.0f : (float)both / (float)any;
        out[(size_t)q * out_stride + i] = sim;
        best = q == 0 ? sim : fmaxf(best, sim);
    }
    if (fused) fused[i] = best;
}

} // namespace

extern "C" int pmx_library_fingerprints(const pmx_library *lib, uint64_t first, uint64_t count, const int32_t *conformer_dev, uint64_t *fingerprint_dev, uint8_t *type_count_dev,
                                        int32_t *status_dev, void *stream_) {
    if (!lib) return pmx_fail(PMX_ERR_INVALID, "pmx_library_fingerprints: null library");
    const pmx_library_info &info = lib->info;
    if (first > info.n_ligands || count > info.n_ligands - first)
        return pmx_fail(PMX_ERR_INVALID, "pmx_library_fingerprints: ligands %llu .. %llu of a library of %llu", (unsigned long long)first, (unsigned long long)(first + count),
                        (unsigned long long)info.n_ligands);
    if (count == 0) return PMX_OK;
    if (!fingerprint_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_library_fingerprints: null fingerprint_dev");
    if (hipSetDevice(lib->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_library_fingerprints: hipSetDevice failed");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    constexpr uint64_t kChunk = 1ull << 30; // ligands per launch (a grid has fewer than 2^31 blocks)
    for (uint64_t at = 0; at < count; at += kChunk) {
        const uint64_t todo = count - at < kChunk ? count - at : kChunk;
        ligand_fp_kernel<<<dim3((unsigned)((todo + kWaves - 1) / kWaves)), dim3(64 * kWaves), 0, stream>>>(
            lib->offsets, lib->data, first + at, todo, conformer_dev ? conformer_dev + at : nullptr, fingerprint_dev + at * kW, type_count_dev ? type_count_dev + at * 8 : nullptr,
            status_dev ? status_dev + at : nullptr);
        PMX_HIPCHECK(hipGetLastError());
    }
    return PMX_OK;
}

extern "C" int pmx_fingerprint_search(const uint64_t *query_dev, uint32_t nq, const uint64_t *fp_dev, uint64_t n, float *out_dev, uint64_t out_stride, float *fused_dev,
                                      int device, void *stream_) {
    if (nq < 1 || nq > PMX_SEARCH_MAX_QUERIES) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_search: 1 to 64 queries");
    if (n > 0x7fffffffull) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_search: more than 2^31 - 1 fingerprints");
    if (out_stride < n) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_search: out_stride is smaller than n");
    if (n == 0) return PMX_OK;
    if (!query_dev || !fp_dev || !out_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_fingerprint_search: null argument");
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_fingerprint_search: hipSetDevice failed");
    search_kernel<<<dim3((unsigned)((n + 255u) / 256u)), dim3(256), 0, static_cast<hipStream_t>(stream_)>>>(query_dev, nq, fp_dev, n, out_dev, out_stride, fused_dev);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
