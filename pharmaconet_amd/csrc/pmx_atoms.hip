// pmx_atoms.hip - the atom store on gfx950: each ligand's heavy atoms resident next to its record (pmx_atoms_upload), and the rows of a
// call gathered from it into the three point-mode arguments of pmx_pose_clash and pmx_pose_refine (pmx_atoms_gather). The format, the
// statuses and the limits are the comment of include/pmx.h; tests/atoms_ref.py restates both in NumPy.
//
// The upload checks every record on the host - offsets, headers against sizes, every element below 128 - so a kernel trusts what it reads.
// size_kernel - a thread per row: the row's status and its number of points, into status_dev[i] and point_off_dev[i + 1].
// scan_kernel - one block of 1024 threads turns the sizes into offsets in place: a thread adds up its run of at most 64 consecutive rows,
//               the runs' totals are scanned through LDS (a wave's by shuffles, the 16 waves' by one wave), the thread writes its run's
//               prefixes. Integer sums: the same whatever the order. 65536 rows of at most 256 points stay below 2^24.
// copy_kernel - one wavefront per row, kWaves per block, nothing shared between the waves: the header is read once per wave (uniform), the
//               lanes take the row's atoms in trips of 64 - the element's radius from the table, the three float32 of the conformer copied.
// No allocation, no synchronisation, no atomic: a row's contents are a copy and do not depend on where it stands.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "pmx.h"
#include "pmx_atoms.h"
#include "pmx_device.h"

namespace {

constexpr int kWaves = 4;
constexpr int kScanThreads = 1024;
constexpr uint32_t kHeader = 8; // u16 n_atoms | u16 n_conf | u32 0

// Where the float32 coordinates of a record of n atoms begin.
__host__ __device__ inline uint32_t xyz_at(uint32_t n) { return (kHeader + n + 3u) & ~3u; }

inline uint64_t record_bytes(uint32_t n, uint32_t C) { return n == 0 ? 16 : ((uint64_t)xyz_at(n) + 12ull * n * C + 15ull) & ~15ull; }

struct GatherArgs {
    const uint64_t *offsets;
    const uint8_t *data;
    const float *table;
    uint64_t n_ligands;
    const uint64_t *ligands;
    const int32_t *conformer;
    uint32_t n;
    uint64_t *point_off;
    float *points;
    float *point_radius;
    int32_t *status;
};

__global__ __launch_bounds__(256) void size_kernel(const GatherArgs a) {
    const uint32_t row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row == 0) a.point_off[0] = 0;
    if (row >= a.n) return;
    const uint64_t lig = a.ligands[row];
    const int c = a.conformer[row];
    int status = PMX_LIGAND_UNSUPPORTED; // (not a ligand of the store, or no atoms kept: nothing further is read)
    uint32_t size = 0;
    if (lig < a.n_ligands) {
        const uint32_t head = *reinterpret_cast<const uint32_t *>(a.data + a.offsets[lig]);
        const uint32_t na = head & 0xFFFFu, C = head >> 16;
        if (na > 0) {
            status = c < 0 || (uint32_t)c >= C ? PMX_LIGAND_KEY_INVALID : PMX_LIGAND_OK;
            if (status == PMX_LIGAND_OK) size = na;
        }
    }
    a.status[row] = status;
    a.point_off[row + 1] = size;
}

// point_off[1 .. n] holds sizes; afterwards their inclusive sums (point_off[0] is 0 already).
__global__ __launch_bounds__(kScanThreads) void scan_kernel(uint64_t *point_off, uint32_t n) {
    __shared__ uint32_t wave_total[kScanThreads / 64];
    const uint32_t t = threadIdx.x, lane = t % 64, wave = t / 64;
    const uint32_t per = (n + kScanThreads - 1) / kScanThreads;
    const uint32_t lo = t * per < n ? t * per : n, hi = lo + per < n ? lo + per : n;
    uint32_t sum = 0;
    for (uint32_t i = lo; i < hi; ++i) sum += (uint32_t)point_off[1 + i];
    // inclusive scan of the threads' sums within the wave
    uint32_t incl = sum;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(incl, d);
        if (lane >= (uint32_t)d) incl += o;
    }
    if (lane == 63) wave_total[wave] = incl;
    __syncthreads();
    if (wave == 0) {
        uint32_t w = lane < kScanThreads / 64 ? wave_total[lane] : 0u;
#pragma unroll
        for (int d = 1; d < kScanThreads / 64; d <<= 1) {
            const uint32_t o = __shfl_up(w, d);
            if (lane >= (uint32_t)d) w += o;
        }
        if (lane < kScanThreads / 64) wave_total[lane] = w; // (inclusive over the waves)
    }
    __syncthreads();
    uint32_t run = (wave ? wave_total[wave - 1] : 0u) + (incl - sum); // what stands before this thread's run
    for (uint32_t i = lo; i < hi; ++i) {
        run += (uint32_t)point_off[1 + i];
        point_off[1 + i] = run;
    }
}

__global__ __launch_bounds__(64 * kWaves) void copy_kernel(const GatherArgs a) {
    const uint32_t row = blockIdx.x * kWaves + __builtin_amdgcn_readfirstlane(threadIdx.x / 64);
    if (row >= a.n) return;
    if (a.status[row] != PMX_LIGAND_OK) return; // (no points: point_off[row + 1] == point_off[row])
    const uint32_t lane = threadIdx.x % 64;
    const uint8_t *rec = a.data + a.offsets[a.ligands[row]];
    const uint32_t head = __builtin_amdgcn_readfirstlane(*reinterpret_cast<const uint32_t *>(rec));
    const uint32_t na = head & 0xFFFFu, C = head >> 16;
    const uint32_t c = (uint32_t)__builtin_amdgcn_readfirstlane(a.conformer[row]);
    const uint64_t o0 = a.point_off[row];
    const uint8_t *element = rec + kHeader;
    const float *xyz = reinterpret_cast<const float *>(rec + xyz_at(na)) + (size_t)c * 3;
    for (uint32_t u = lane; u < na; u += 64) {
        const float *x = xyz + (size_t)u * C * 3;
        float *p = a.points + (o0 + u) * 3;
        p[0] = x[0];
        p[1] = x[1];
        p[2] = x[2];
        a.point_radius[o0 + u] = a.table[element[u]];
    }
}

} // namespace

extern "C" int pmx_atoms_upload(const pmx_atoms_view *view, const float radius_of_element[128], int device, pmx_atoms **out) {
    if (!out) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: null out");
    *out = nullptr;
    if (!view || !radius_of_element) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: null view or radius table");
    const uint64_t N = view->n_ligands;
    if (!view->offsets || (N > 0 && !view->data)) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: null offsets or data");
    if (N >= (1ull << 40)) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: %llu ligands", (unsigned long long)N);
    const uint64_t *off = view->offsets;
    if (off[0] != 0) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: offsets[0] is %llu, not 0", (unsigned long long)off[0]);
    pmx_atoms_info info{};
    info.n_ligands = N;
    for (uint64_t i = 0; i < N; ++i) {
        const uint64_t lo = off[i], hi = off[i + 1];
        if (hi < lo || lo % 16 != 0 || hi % 16 != 0 || hi - lo < 16)
            return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: record %llu spans %llu .. %llu: offsets must rise in steps of 16 bytes", (unsigned long long)i,
                            (unsigned long long)lo, (unsigned long long)hi);
        const uint8_t *rec = view->data + lo;
        uint16_t na, C;
        uint32_t zero;
        std::memcpy(&na, rec, 2);
        std::memcpy(&C, rec + 2, 2);
        std::memcpy(&zero, rec + 4, 4);
        if (na > PMX_MAX_LIGAND_ATOMS || C > PMX_MAX_CONFORMERS || zero != 0 || (na > 0 && C == 0))
            return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: record %llu has a header of %u atoms and %u conformers (at most %d and %d)", (unsigned long long)i,
                            (unsigned)na, (unsigned)C, PMX_MAX_LIGAND_ATOMS, PMX_MAX_CONFORMERS);
        if (hi - lo != record_bytes(na, C))
            return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: record %llu is %llu bytes, its header says %llu", (unsigned long long)i, (unsigned long long)(hi - lo),
                            (unsigned long long)record_bytes(na, C));
        for (uint32_t u = 0; u < na; ++u)
            if (rec[kHeader + u] > 127) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_upload: record %llu, atom %u: element %u above 127", (unsigned long long)i, u, (unsigned)rec[kHeader + u]);
        if (na == 0) ++info.n_empty;
        if ((int32_t)na > info.max_atoms) info.max_atoms = na;
    }
    info.n_bytes = off[N];
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_atoms_upload: hipSetDevice failed");
    pmx_atoms *a = new pmx_atoms;
    a->device = device;
    a->info = info;
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&a->offsets), sizeof(uint64_t) * (N + 1));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&a->data), info.n_bytes ? info.n_bytes : 16);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void **>(&a->radius), sizeof(float) * 128);
    if (e == hipSuccess) e = hipMemcpy(a->offsets, off, sizeof(uint64_t) * (N + 1), hipMemcpyHostToDevice);
    if (e == hipSuccess && info.n_bytes) e = hipMemcpy(a->data, view->data, info.n_bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(a->radius, radius_of_element, sizeof(float) * 128, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (a->offsets) (void)hipFree(a->offsets);
        if (a->data) (void)hipFree(a->data);
        if (a->radius) (void)hipFree(a->radius);
        delete a;
        return pmx_fail(e == hipErrorOutOfMemory ? PMX_ERR_OOM : PMX_ERR_HIP, "pmx_atoms_upload: %s", hipGetErrorString(e));
    }
    *out = a;
    return PMX_OK;
}

extern "C" int pmx_atoms_info_get(const pmx_atoms *atoms, pmx_atoms_info *info) {
    if (!atoms || !info) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_info_get: null store or info");
    *info = atoms->info;
    return PMX_OK;
}

extern "C" int pmx_atoms_destroy(pmx_atoms *atoms) {
    if (!atoms) return PMX_OK;
    if (hipSetDevice(atoms->device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_atoms_destroy: hipSetDevice failed");
    if (atoms->offsets) (void)hipFree(atoms->offsets);
    if (atoms->data) (void)hipFree(atoms->data);
    if (atoms->radius) (void)hipFree(atoms->radius);
    delete atoms;
    return PMX_OK;
}

extern "C" int pmx_atoms_gather(const pmx_atoms *atoms, const uint64_t *ligands_dev, const int32_t *conformer_dev, uint32_t n, uint64_t cap_points, uint64_t *point_off_dev,
                                float *points_dev, float *point_radius_dev, int32_t *status_dev, void *stream_) {
    if (!atoms) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_gather: null store");
    if (n > PMX_EXPLAIN_MAX) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_gather: %u rows, at most %d", n, PMX_EXPLAIN_MAX);
    const uint64_t need = (uint64_t)n * (uint64_t)atoms->info.max_atoms;
    if (cap_points < need)
        return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_gather: cap_points %llu, %u rows of at most %d atoms need %llu", (unsigned long long)cap_points, n, atoms->info.max_atoms,
                        (unsigned long long)need);
    if (!point_off_dev) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_gather: null point_off_dev");
    if (n > 0 && (!ligands_dev || !conformer_dev || !points_dev || !point_radius_dev || !status_dev)) return pmx_fail(PMX_ERR_INVALID, "pmx_atoms_gather: null input or output");
    PMX_HIPCHECK(hipSetDevice(atoms->device));
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    if (n == 0) {
        PMX_HIPCHECK(hipMemsetAsync(point_off_dev, 0, sizeof(uint64_t), stream));
        return PMX_OK;
    }
    const GatherArgs a{atoms->offsets, atoms->data, atoms->radius, atoms->info.n_ligands, ligands_dev, conformer_dev, n, point_off_dev, points_dev, point_radius_dev, status_dev};
    size_kernel<<<dim3((n + 255) / 256), dim3(256), 0, stream>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    scan_kernel<<<dim3(1), dim3(kScanThreads), 0, stream>>>(point_off_dev, n);
    PMX_HIPCHECK(hipGetLastError());
    copy_kernel<<<dim3((n + kWaves - 1) / kWaves), dim3(64 * kWaves), 0, stream>>>(a);
    PMX_HIPCHECK(hipGetLastError());
    return PMX_OK;
}
