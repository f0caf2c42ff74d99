// pmx_scan.h - what the two makers of a library's offsets share (the device packer, pmx_pack_device.hip, and the record gather,
// pmx_select.hip): the kernel behind hipcub's exclusive scan of the record sizes.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pmx {

// offsets[n] = offsets[n - 1] + sizes[n - 1] (the exclusive scan leaves the end of the last record out); total_out (may be null) gets a copy.
static __global__ void close_offsets_kernel(const uint64_t *sizes, uint64_t *offsets, uint64_t n, uint64_t *total_out) {
    if (threadIdx.x == 0 && blockIdx.x == 0) {
        const uint64_t total = n ? offsets[n - 1] + sizes[n - 1] : 0;
        offsets[n] = total;
        if (total_out) *total_out = total;
    }
}

} // namespace pmx
