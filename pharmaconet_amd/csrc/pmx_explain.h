// pmx_explain.h - launchers of the explain kernels (pmx_explain.hip), called by pmx_explain(), pmx_explain_constrained() and pmx_explain_modes() in pmx_api.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <stdint.h>

#include "pmx.h"
#include "pmx_screen_layout.h"

namespace pmx_xpl {
// Where one call's answers go (device pointers, see pmx_explain in include/pmx.h); row i belongs to ligands[i].
struct Args {
    const uint64_t *ligands; // [n] library indices
    uint32_t n;
    uint32_t n_modes;  // 1 .. PMX_MAX_MODES leaves per conformer: 1 for pmx_explain and pmx_explain_constrained
    double *conf_max;  // [n][n_modes][PMX_MAX_CONFORMERS]
    uint8_t *match;    // [n][n_modes][PMX_MAX_CONFORMERS][PMX_MAX_LEVELS]
    uint8_t *levels;   // [n][PMX_MAX_LEVELS]
    int32_t *best;     // [n]
    int32_t *status;   // [n]
    pmx_match_constraint con; // which leaves may hold a maximum (read by the constrained kernels only)
};
// Dynamic LDS of the explain kernel of shape G for a model of K clusters and a library of at most max_nodes nodes per ligand
// (0 for a G this side does not know); the constrained kernels keep two more 128-bit words per tree level, and every kernel n_modes
// totals per conformer lane (4 KB at 64 lanes and 8 modes; the keys, 10 KB there, live in the row's output block instead: a leaf
// enters a list rarely after the first few).
size_t lds_bytes(int G, int K, int max_nodes, bool constrained, int n_modes);
// `p` with p.mode as the pass: 0 the listed ligands with tables in per-wave slices, 1 the large-slice pass, 2 / 3 the arena passes.
// `constrained`: the kernels that test every leaf against a.con; without it a.con is not read. Returns false when G is not a lane
// count the kernels are built for.
bool launch(int G, bool tails, bool constrained, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p, const Args &a);
void launch_init(const Args &a, hipStream_t stream);  // rows as for a ligand without levels: maxima 0, no match, no levels (every mode's)
void launch_fixup(const Args &a, hipStream_t stream); // rows of ligands with a non-zero status: maxima NaN (every mode's), best conformer -1
} // namespace pmx_xpl
