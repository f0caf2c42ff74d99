// pmx_model_tables.h - everything pmx_model_create computes from a pmx_model_desc, as host arrays: the tables the kernels read (DevModel,
// ScreenParams, fn_build_kernel) before they are uploaded. Host only, no HIP header: the unit is part of libpmx.so and of the host-only
// libpmx_pack.so, where the CPU tests reach it through the pmxt_* hook below. It must be compiled with -ffp-contract=off.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pmx.h"

namespace pmx {

// float2 and float4 of the device side, member for member (pmx_api.hip asserts size and layout).
struct F2 {
    float x, y;
};
struct F4 {
    float x, y, z, w;
};

constexpr size_t kFnCellBytes = 32; // sizeof(FnCell), pmx_screen_layout.h: the size limit of the tabulated pair functions

struct ModelTables {
    int32_t Nm = 0, K = 0;
    int32_t symmetric = 1;          // edge[m][n] == edge[n][m] bit for bit
    std::vector<F4> edge;           // [Nm * Nm] {mean, s, T, std} (DevModel, pmx_device.h)
    std::vector<uint8_t> node_type; // [PMX_MAX_MODEL_NODES]
    std::vector<uint64_t> tclus;    // [128][2]
    std::vector<F2> cpair;          // [K * K]
    std::vector<F2> cwin;           // [K * K] hull of the edge windows of a cluster pair's node pairs; {+inf, -inf}: none
    // node subsets: (model cluster, ligand type mask) -> the cluster's nodes of those types (graph_match.py:148-150)
    uint32_t NS = 0;                // distinct subsets; subset 0 is the empty one
    std::vector<uint16_t> sidtab;   // [max(K, 1) * 128] subset of (cluster, mask)
    std::vector<uint32_t> sub_off;  // [NS + 1] the nodes of subset s are sub_nodes[sub_off[s] .. sub_off[s + 1]), ascending
    std::vector<uint8_t> sub_nodes; // (never empty: one 0 when no subset has a node)
    // pass windows of the tabulated pair functions on a grid of ncell cells of width h (the last cell stands for every distance beyond)
    uint32_t NF = 0, ncell = 0;     // functions: NS * (NS + 1) / 2 for a symmetric model ((sa, sb), sb <= sa, at sa * (sa + 1) / 2 + sb), else NS * NS
    float h = 0.f;
    std::vector<F2> win;            // [NF][ncell] {lo, hi}: the distances of the cell that pass the majority test of match_utils.py:55-61;
                                    // {inf, inf}: none; {NaN, NaN}: not one interval (the kernel counts the terms)
    uint64_t n_complex_cells = 0;   // the NaN cells of win
    // exact pass window of every model edge: the floats d >= 0 with abs((d - mean) / std) < 2 in float32 are wlo <= d <= whi (wok == 0: none)
    std::vector<float> wlo, whi;    // [Nm * Nm]
    std::vector<uint8_t> wok;
};

// Validates the description and fills `out`. PMX_OK, or PMX_ERR_INVALID with the thread's message set (pmx_error.h).
int build_model_tables(const pmx_model_desc *d, ModelTables *out);

} // namespace pmx

// Test hook (not part of include/pmx.h): the tables of a description, without a device.
extern "C" {
typedef struct pmxt_tables pmxt_tables;
typedef struct {
    int32_t Nm, K, symmetric;
    uint32_t NS, NF, ncell;
    float h;
    uint64_t n_complex_cells;
    // the arrays of ModelTables with their element counts (F4 / F2 count as one element)
    const float *edge, *cpair, *cwin, *win, *wlo, *whi;
    const uint8_t *node_type, *sub_nodes, *wok;
    const uint64_t *tclus;
    const uint16_t *sidtab;
    const uint32_t *sub_off;
    uint64_t n_edge, n_cpair, n_cwin, n_win, n_node_type, n_sub_nodes, n_tclus, n_sidtab, n_sub_off;
} pmxt_tables_view;
int pmxt_tables_create(const pmx_model_desc *desc, pmxt_tables **out);
int pmxt_tables_view_get(const pmxt_tables *t, pmxt_tables_view *view);
int pmxt_tables_destroy(pmxt_tables *t);
}
