// pmx_screen_lds.h - the part of the screening path's layouts that depends on a compile-time switch, and therefore stays a type of its
// own in every namespace the kernels are compiled into: a wavefront's LDS (WaveShape, wave_shape, through PMX_TC_LEVELS) and how a kernel
// reads ScreenParams::flags (PMX_WFLAGS, through PMX_DEBUG_KERNELS). Host and device. The host planner (plan_pocket, pmx_api.hip) and
// pmx_xpl::lds_bytes (pmx_explain.hip) size launches with their own unit's wave_shape, so tools/build_variant.py compiles the units that
// do (pmx_api.hip, pmx_screen_debug.hip, pmx_explain.hip) with the variant's flags. The switch-free layouts: pmx_screen_layout.h.
#pragma once
#include "pmx_screen_layout.h"

// The screening code is compiled five times, each into a namespace of its own (PMX_NS). libpmx's own kernels (namespace pmx, pmx_api.hip)
// know two PMX_TREE_FLAGS switches - no budget (2) and tables alone (16384) - and read every other bit as zero, so the walker and the table
// loops carry none of the validation switches (1.5 % of the pass; as a template parameter in one translation unit the two sets of kernels
// cost each other registers). pmx_screen_debug.hip compiles pmx_screen.hip again as namespace pmx_dbg with every switch live; a call with
// any other bit set launches those. pmx_explain.hip compiles the table phase alone as namespace pmx_x, under a walker of its own;
// pmx_rows.hip (pmx_r) and pmx_pose_fit.hip (pmx_f) take its record and wavefront helpers only and never touch a WaveShape.
#ifndef PMX_NS
#define PMX_NS pmx
#endif
#ifdef PMX_DEBUG_KERNELS
#define PMX_WFLAGS(p) ((p).flags)
#else
#define PMX_WFLAGS(p) ((p).flags & PMX_PRODUCT_FLAGS)
#endif

// The one tuning constant that changes a layout (WaveShape: the children cache is PMX_TC_LEVELS x 520 bytes of a wavefront's LDS, and the
// host sizes launches from wave_shape().bytes): the frames whose children's totals are cached.
#ifndef PMX_TC_LEVELS
#define PMX_TC_LEVELS 4 // ([MI355X] 3 -> 4: 101.0 -> 100.2-100.8 ms per pass; 5: 107.1, the LDS of a wave rounds up to 7 168 bytes, 22 waves per CU; 2 / 1: 107.7 / 107.5 against 105.4)
#endif

namespace PMX_NS {
using namespace pmx; // (pmx_device.h, pmx_screen_layout.h)

// ------------------------------------------------------------------------------------------- LDS of a wave
// Frames nl - 3 .. nl - 2 - kTcLevels keep their children's totals in LDS: when the walker comes back to such a frame the
// remaining candidates are taken from there instead of being evaluated again (a third of all passes were re-evaluations).
constexpr int kTcLevels = PMX_TC_LEVELS;
static_assert(kTcLevels >= 1 && kTcLevels <= 8, "cache slot number is three bits of Walk::hk");
template <int G>
struct WaveShape {
    uint32_t kp;     // candidates per level, padded
    uint32_t nc_cap; // node-candidate entries
    uint32_t off_cand, off_lcnt, off_nc, off_tot, off_pool, off_stat, off_task, off_tch, off_tc, off_cb, off_ub, bytes;
};
template <int G>
__host__ __device__ inline WaveShape<G> wave_shape(int K, int max_nodes) {
    WaveShape<G> w;
    w.kp = (uint32_t)((K + 3) & ~3);
    w.nc_cap = w.kp * (uint32_t)((max_nodes + 3) & ~3);
    uint32_t o = 512; // fixed part: type masks, level arrays
    w.off_cand = o;
    o += PMX_MAX_LEVELS * w.kp;
    w.off_lcnt = o;
    o += PMX_MAX_LEVELS * w.kp;
    o = (o + 15u) & ~15u;
    w.off_nc = o;
    o += w.nc_cap * 2;
    o = (o + 15u) & ~15u;
    w.off_tot = o;
    if (totals_in_lds<G>()) o += (PMX_MAX_LEVELS + 1) * G * 8;
    w.off_pool = o;
    o += G * 8;
    w.off_stat = o; // the wave's statistics (kept out of the registers)
    o += 208; // sizeof(WaveStats) (pmx_screen_tables.h, which asserts it)
    w.off_task = o; // subtree record of the root of the ligand in work
    o += task_rec_bytes<G>();
    o = (o + 15u) & ~15u;
    w.off_tch = o; // totals of a frame's children (fused last two levels)
    // path_bound() keeps the tested child's totals in the first G entries and nothing else of this block: its level maxima live behind them
    // (the fused block, which fills all 64 entries, and path_bound() never run inside one another) - the room that saves is a fourth cached level
    {
        uint32_t blk = 64 * 8;
        if (cand_bounds<G>()) blk = blk > (uint32_t)(G * 8 + PMX_MAX_LEVELS * G * 4) ? blk : (uint32_t)(G * 8 + PMX_MAX_LEVELS * G * 4);
        o += blk;
    }
    w.off_tc = o; // the children's totals of the kTcLevels deepest unfused frames + their validity ballots
    if (totals_in_lds<G>()) o += kTcLevels * (64 * 8 + 8);
    w.off_cb = o; // candidates of a filtered frame that are still to visit, one 64-bit set per level (32 / 64 conformer lanes)
    if (64 / G <= 2) o += PMX_MAX_LEVELS * 8;
    w.off_ub = w.off_tch + G * 8; // path_bound(): the most a level can add, per conformer (inside the block of the children's totals, see above)
    w.bytes = o;
    return w;
}

} // namespace PMX_NS
