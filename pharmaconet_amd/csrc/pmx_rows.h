// pmx_rows.h - launchers of the row kernels (pmx_rows.hip): attribution, rigid fit and hotspot shares of listed (ligand, conformer, key) rows, called by
// pmx_attribute(), pmx_align() and pmx_hotspots() in pmx_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <stdint.h>

#include "pmx_screen_layout.h"

namespace pmx_rows {
// One call's rows and what every row kernel says about a row (device pointers); row i is ligands[i] at conformer[i] under key[i].
struct Rows {
    const uint64_t *ligands;  // [n] library indices
    const int32_t *conformer; // [n]
    const uint8_t *key;       // [n][PMX_MAX_LEVELS] model cluster per tree level, 0xFF for None
    uint32_t n;
    uint8_t *levels;  // [n][PMX_MAX_LEVELS]
    int32_t *status;  // [n]
    uint32_t *cursor; // the call's row cursor, zero when the kernel starts
};
// Where the answers of pmx_attribute go (include/pmx.h).
struct AttributeArgs {
    Rows rows;
    double *total;   // [n]
    double *node;    // [n][PMX_MAX_LIGAND_NODES]
    float *entry;    // [n][PMX_MAX_LEVELS][PMX_MAX_LEVELS]
    uint16_t *fails; // [n][PMX_MAX_LEVELS][PMX_MAX_LEVELS]
};
// The model nodes' centres and where the answers of pmx_align go (include/pmx.h).
struct AlignArgs {
    Rows rows;
    const double *center; // [Nm][3]
    double *rot;          // [n][9]
    double *trans;        // [n][3]
    double *fit;          // [n][8]
    double *node;         // [n][PMX_MAX_LIGAND_NODES]
    int32_t *count;       // [n][2]
};
// Where the answers of pmx_hotspots go (include/pmx.h).
struct HotspotArgs {
    Rows rows;
    double *total;         // [n]
    double *hotspot;       // [n][PMX_MAX_MODEL_NODES]
    uint32_t *terms;       // [n][PMX_MAX_MODEL_NODES]
    uint32_t *pass;        // [n][PMX_MAX_MODEL_NODES]
    uint64_t *fingerprint; // [n][PMX_FINGERPRINT_WORDS]
};
enum Kind { kAttribute, kAlign, kHotspots };
// Static LDS of one wavefront of the kernel: how many fit a compute unit.
size_t lds_bytes(Kind kind);
// `p`: the model, the library, the node subsets and the weights filled in (row_params, pmx_handles.h); the arguments pick the kernel.
void launch(unsigned blocks, hipStream_t stream, const pmx::ScreenParams &p, const AttributeArgs &a);
void launch(unsigned blocks, hipStream_t stream, const pmx::ScreenParams &p, const AlignArgs &a);
void launch(unsigned blocks, hipStream_t stream, const pmx::ScreenParams &p, const HotspotArgs &a);
} // namespace pmx_rows
