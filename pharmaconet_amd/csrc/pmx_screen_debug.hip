// pmx_screen_debug.hip - pmx_screen.hip once more, as namespace pmx_dbg, with every PMX_TREE_FLAGS switch compiled in: the kernels
// behind the validation settings of the tests (no bounds, no fused levels, no cache, term-by-term items, ...) and the phase studies
// of tools/. libpmx's own kernels (namespace pmx) carry none of these switches; see the note on PMX_NS in pmx_screen_lds.h.
#include <hip/hip_runtime.h>

#define PMX_DEBUG_KERNELS 1
#define PMX_NS pmx_dbg
#include "pmx_screen.hip"
#include "pmx_debug.h"

namespace pmx_debug {

bool launch_ligand(int G, bool exact, bool tails, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p) {
    return pmx::with_lanes(G, [&](auto g) {
        constexpr int L = decltype(g)::value;
        if (exact) pmx_dbg::ligand_kernel<L, true, false><<<dim3(blocks), dim3(64), lds, stream>>>(p);
        else if (tails) pmx_dbg::ligand_kernel<L, false, true><<<dim3(blocks), dim3(64), lds, stream>>>(p);
        else pmx_dbg::ligand_kernel<L, false, false><<<dim3(blocks), dim3(64), lds, stream>>>(p);
    });
}

bool launch_task(int G, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p) {
    return pmx::with_lanes(G, [&](auto g) { pmx_dbg::task_kernel<decltype(g)::value><<<dim3(blocks), dim3(64), lds, stream>>>(p); });
}

} // namespace pmx_debug
