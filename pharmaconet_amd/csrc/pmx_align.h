// pmx_align.h - launcher of the rigid-fit kernel (pmx_align.hip), called by pmx_align() in pmx_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <stdint.h>

namespace pmx_aln {
// One call's rows and where their answers go (device pointers, see pmx_align in include/pmx.h); row i is ligands[i] at conformer[i] under key[i].
struct Args {
    const uint64_t *ligands;  // [n] library indices
    const int32_t *conformer; // [n]
    const uint8_t *key;       // [n][PMX_MAX_LEVELS] model cluster per tree level, 0xFF for None
    uint32_t n;
    const double *center; // [Nm][3] the model nodes' centres
    double *rot;          // [n][9]
    double *trans;        // [n][3]
    double *fit;          // [n][8]
    double *node;         // [n][PMX_MAX_LIGAND_NODES]
    int32_t *count;       // [n][2]
    uint8_t *levels;      // [n][PMX_MAX_LEVELS]
    int32_t *status;      // [n]
    uint32_t *cursor;     // the call's row cursor, zero when the kernel starts
};
// Static LDS of one wavefront of the kernel: how many fit a compute unit.
size_t lds_bytes();
// `params`: the caller's pmx::ScreenParams with the model, the library, the node subsets and the weights filled in (same source and
// layout; `bytes` is checked against this side's sizeof). Returns false when the size is not the one this side knows.
bool launch(unsigned blocks, hipStream_t stream, const void *params, size_t bytes, const Args &a);
} // namespace pmx_aln
