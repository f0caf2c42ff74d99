// pmx_debug.h - launchers of the screening kernels compiled with every PMX_TREE_FLAGS switch live (pmx_screen_debug.hip).
// pmx_api.hip calls them when a bit outside PMX_PRODUCT_FLAGS is set; libpmx's own kernels read those bits as zero.
#pragma once
#include <hip/hip_runtime.h>

#include "pmx_screen_layout.h"

namespace pmx_debug {
// G = lanes per slot (1 .. 64, a power of two). Returns false when G is not a lane count the kernels are built for.
bool launch_ligand(int G, bool exact, bool tails, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p);
bool launch_task(int G, unsigned blocks, unsigned lds, hipStream_t stream, const pmx::ScreenParams &p);
} // namespace pmx_debug
