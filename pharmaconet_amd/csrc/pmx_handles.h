// pmx_handles.h - what stands behind the opaque pmx_model and pmx_library of include/pmx.h, for the units of libpmx.so that take such a
// handle (host only): they read a library's device, counts and buffers and a model's tables here, not through a function of another
// unit. pmx_api.hip makes and destroys both; struct pmx_pocket is pmx_pose.h's.
#pragma once
#include <mutex>
#include <vector>

#include "pmx_screen_layout.h"

struct FnEntry { // tabulated pair functions for one set of type weights
    pmx::Weights W;
    pmx::FnCell *cells = nullptr;
    hipEvent_t ready = nullptr; // recorded after fn_build_kernel on the stream that built it
    uint64_t stamp = 0;
};

// The tables of pmx_model_tables.cpp in one device allocation; every pointer below and in `dm` points into `blob`.
struct pmx_model {
    int device;
    pmx::DevModel dm;
    void *blob;
    uint8_t node_type[PMX_MAX_MODEL_NODES]; // host copy
    // node subsets and tabulated pair functions (pmx_screen_layout.h FnTable, pmx_screen_tables.h fn_build_kernel)
    uint32_t NS = 0, NF = 0, ncell = 0;
    float h = 0.f;
    const uint16_t *sidtab = nullptr;  // [K * 128]
    const uint32_t *sub_off = nullptr;  // [NS + 1]: the nodes of subset s are sub_nodes[sub_off[s] .. sub_off[s + 1]), ascending
    const uint8_t *sub_nodes = nullptr;
    const float2 *win = nullptr;        // [NF * ncell] exact pass windows
    std::mutex fn_mu;
    std::vector<FnEntry> fn;
    uint64_t fn_stamp = 0;
};

struct pmx_library {
    int device;
    pmx::DevLibrary dl;
    uint64_t *offsets;
    uint8_t *data;
    bool owns; // false: the caller's device buffers, adopted as they are (pmx_library_view.on_device == 2)
    pmx_library_info info;
};

namespace pmx {

inline Weights to_weights(const float weights[PMX_NUM_TYPES]) {
    Weights W;
    for (int t = 0; t < PMX_NUM_TYPES; ++t) W.w[t] = weights[t];
    return W;
}

// What a row kernel reads of a model, a library and the weights: a ScreenParams with those filled in and nothing else.
inline ScreenParams row_params(const pmx_model *model, const pmx_library *lib, const float weights[PMX_NUM_TYPES]) {
    ScreenParams p{};
    p.M = model->dm;
    p.lib = lib->dl;
    p.sidtab = model->sidtab;
    p.sub_off = model->sub_off;
    p.sub_nodes = model->sub_nodes;
    p.W = to_weights(weights);
    return p;
}

} // namespace pmx
