// pmx_select.hip - sub-libraries on the device: pmx_library_select gathers the packed records of a list of ligands into a new library.
//
// The score pass takes a contiguous range of a resident library; everything a user does after a screen is about a list (the best hits
// against other pockets, the survivors of a filter, the hits kept for the next campaign). The gather makes a list a library again, inside
// HBM, so the pass itself needs no index list. Three launches and one small read, on the caller's stream:
//
//   sizes_kernel   one thread per listed index: the record's size, or 0 and a count for an index outside the library (the first such
//                  position by a 64-bit atomicMin)
//   (exclusive scan of the sizes: hipcub; close_offsets_kernel of pmx_scan.h, which also leaves the total next to the two counters)
//   the host reads {bad indices, first bad position, total bytes} - the one wait of the call
//   copy_kernel    one wavefront per record: records start on 16-byte boundaries and are multiples of 16 bytes (pmx_library_upload checks
//                  both), so a record is moved as uint4, 16 bytes per lane per trip, addressed with 64-bit byte offsets (an output may exceed 4 GiB)
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <cstdio>
#include <mutex>

#include "pmx.h"
#include "pmx_device.h"
#include "pmx_handles.h"
#include "pmx_scan.h"

namespace {

// counters[0]: indices outside the library; counters[1]: the first position that holds one; counters[2]: total bytes (close_offsets_kernel)
__global__ __launch_bounds__(256) void sizes_kernel(const uint64_t *lib_offsets, uint64_t n_ligands, const uint64_t *indices, uint64_t n, uint64_t *sizes,
                                                    unsigned long long *counters) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint64_t idx = indices[i];
    if (idx >= n_ligands) {
        sizes[i] = 0;
        atomicAdd(&counters[0], 1ull);
        atomicMin(&counters[1], (unsigned long long)i);
        return;
    }
    sizes[i] = lib_offsets[idx + 1] - lib_offsets[idx];
}

constexpr int kWavesPerBlock = 4;

// Wavefront r copies record indices[r] to offsets_out[r]. (Every listed index is inside the library: the host has read the counters.)
__global__ __launch_bounds__(64 * kWavesPerBlock) void copy_kernel(const uint64_t *lib_offsets, const uint8_t *lib_data, const uint64_t *indices, uint64_t n,
                                                                   const uint64_t *offsets_out, uint8_t *data_out) {
    const uint64_t r = (uint64_t)blockIdx.x * kWavesPerBlock + threadIdx.x / 64;
    if (r >= n) return;
    const uint32_t lane = threadIdx.x % 64;
    const uint64_t idx = indices[r];
    const uint64_t from = lib_offsets[idx], bytes = lib_offsets[idx + 1] - from;
    const uint4 *src = reinterpret_cast<const uint4 *>(lib_data + from);
    uint4 *dst = reinterpret_cast<uint4 *>(data_out + offsets_out[r]);
    const uint64_t nvec = bytes / 16;
    for (uint64_t v = lane; v < nvec; v += 64) dst[v] = src[v];
}

// Work buffers (sizes, scan scratch, the counters) kept from call to call, one set per device, as the packer keeps its own (PackWork): a
// call holds its device's lock while it runs, and it ends with the host waiting for its stream - the scan and both counters are done
// with when the lock is released, and the record copy reads the caller's buffers only. So a call made on another stream needs no event
// to start behind the one before it: whatever that call left on the device does not touch these buffers.
struct SelectWork {
    std::mutex mu;
    pmx::DevBuf sizes, scan, counters;
};
constexpr int kMaxDevices = 64;
SelectWork g_work[kMaxDevices];

bool overlap(const void *a, uint64_t na, const void *b, uint64_t nb) {
    const uintptr_t pa = reinterpret_cast<uintptr_t>(a), pb = reinterpret_cast<uintptr_t>(b);
    return na && nb && pa < pb + nb && pb < pa + na;
}

} // namespace

extern "C" int pmx_library_select(const pmx_library *lib, const uint64_t *indices_dev, uint64_t n, uint64_t *offsets_out_dev, uint8_t *data_out_dev,
                                  uint64_t data_cap, uint64_t *data_bytes, void *stream_) {
    if (!lib || !offsets_out_dev || !data_bytes || (n && !indices_dev) || (!data_out_dev && data_cap)) return pmx_fail(PMX_ERR_INVALID, "pmx_library_select: null argument");
    hipStream_t stream = static_cast<hipStream_t>(stream_);
    const int device = lib->device;
    if (hipSetDevice(device) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_library_select: hipSetDevice failed");
    *data_bytes = 0;
    if (n == 0) {
        if (hipMemsetAsync(offsets_out_dev, 0, 8, stream) != hipSuccess) return pmx_fail(PMX_ERR_HIP, "pmx_library_select: memset failed");
        return PMX_OK;
    }
    if (n > 0x7fffffffull) return pmx_fail(PMX_ERR_INVALID, "pmx_library_select: more than 2^31 - 1 indices in one call");
    if (device < 0 || device >= kMaxDevices) return pmx_fail(PMX_ERR_INVALID, "pmx_library_select: device index out of range");
    const pmx_library_info &info = lib->info;
    const uint64_t *const lib_offsets = lib->offsets;
    const uint8_t *const lib_data = lib->data;
    if (overlap(offsets_out_dev, (n + 1) * 8, lib_offsets, (info.n_ligands + 1) * 8) || overlap(offsets_out_dev, (n + 1) * 8, lib_data, info.n_bytes) ||
        overlap(data_out_dev, data_cap, lib_offsets, (info.n_ligands + 1) * 8) || overlap(data_out_dev, data_cap, lib_data, info.n_bytes))
        return pmx_fail(PMX_ERR_INVALID, "pmx_library_select: the output overlaps the source library's buffers");
    SelectWork &w = g_work[device];
    std::lock_guard<std::mutex> lock(w.mu);
    size_t scan_need = 0;
    (void)hipcub::DeviceScan::ExclusiveSum(nullptr, scan_need, (const uint64_t *)nullptr, (uint64_t *)nullptr, (int)n, stream);
    hipError_t e = w.sizes.grow(n * 8, stream);
    if (e == hipSuccess) e = w.scan.grow(scan_need ? scan_need : 8, stream);
    if (e == hipSuccess) e = w.counters.grow(3 * 8, stream);
    PMX_HIPCHECK(e);
    uint64_t *sizes = w.sizes.as<uint64_t>();
    unsigned long long *counters = w.counters.as<unsigned long long>();
    e = hipMemsetAsync(counters, 0, 8, stream);
    if (e == hipSuccess) e = hipMemsetAsync(counters + 1, 0xFF, 8, stream);
    PMX_HIPCHECK(e);
    sizes_kernel<<<dim3((unsigned)((n + 255) / 256)), dim3(256), 0, stream>>>(lib_offsets, info.n_ligands, indices_dev, n, sizes, counters);
    size_t scan_bytes = w.scan.bytes;
    e = hipcub::DeviceScan::ExclusiveSum(w.scan.ptr, scan_bytes, sizes, offsets_out_dev, (int)n, stream);
    if (e == hipSuccess) {
        pmx::close_offsets_kernel<<<1, 64, 0, stream>>>(sizes, offsets_out_dev, n, reinterpret_cast<uint64_t *>(counters + 2));
        e = hipGetLastError();
    }
    unsigned long long got[3] = {0, 0, 0};
    if (e == hipSuccess) e = hipMemcpyAsync(got, counters, sizeof(got), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    PMX_HIPCHECK(e);
    if (got[0])
        return pmx_fail(PMX_ERR_INVALID, "pmx_library_select: %llu of %llu indices are outside the library's %llu ligands, the first at position %llu", got[0],
                        (unsigned long long)n, (unsigned long long)info.n_ligands, got[1]);
    *data_bytes = got[2];
    if (!data_out_dev) return PMX_OK; // sizing call
    if (got[2] > data_cap) return pmx_fail(PMX_ERR_INVALID, "pmx_library_select: data_out too small (data_bytes holds the size needed)");
    copy_kernel<<<dim3((unsigned)((n + kWavesPerBlock - 1) / kWavesPerBlock)), dim3(64 * kWavesPerBlock), 0, stream>>>(lib_offsets, lib_data, indices_dev, n, offsets_out_dev,
                                                                                                                  data_out_dev);
    e = hipGetLastError();
    PMX_HIPCHECK(e);
    return PMX_OK;
}

// pmx_release_workspaces: the gather's buffers of `device` (the device is current and idle).
int pmx_select_release(int device) {
    if (device < 0 || device >= kMaxDevices) return PMX_OK;
    SelectWork &w = g_work[device];
    std::lock_guard<std::mutex> lock(w.mu); // a call that is running finishes first
    for (pmx::DevBuf *b : {&w.sizes, &w.scan, &w.counters}) b->release();
    return PMX_OK;
}
