// Launch geometry of the separate grid kernels (k_grid, k_grid<true>, k_grid_grad) from the length of the active list.  Plain C++: the engine's host side
// includes it, and tests/csrc/grid_launch_test.cpp builds it for the host with a main of its own.
//
// The kernels have two roads (grid_body / grid_grad_body in fe_engine.hip): a list of at most 4 x gridDim.x entries gives every entry a wave of its own, one round
// trip to the entry and one to its slabs; a longer list is walked eight candidates per wave and round, one dependent slab trip per marked entry.  Which road a launch
// takes is decided on the device from meta[2] and gridDim.x; the host only chooses gridDim.x, from a length the last sort sent it (ListLenOut) -- a hint that may be
// late (the forward pass is enqueued ahead of the GPU) and is never waited for.  Too small a launch means the long road, too large a one means waves that read the
// length and leave.  What the thresholds below were measured at: profiles/grid_launch_geometry.txt, DESIGN.md section 10.
#ifndef FE_GRID_LAUNCH_H
#define FE_GRID_LAUNCH_H

enum { FE_GL_NONE = 0, FE_GL_LAGGED = 1, FE_GL_EXACT = 2, FE_GL_FORCED = 3 };      // where a launch's length came from (fe_get_work_stats [25] / [28])

#define FE_GL_FIXED_WGS 1024        // the fixed geometry: one round of the chip's resident workgroups (four per CU); what a launch without a hint gets
#define FE_GL_FLOOR_WGS 512         // no launch below this: the shortest lists measured no faster with fewer workgroups
#define FE_GL_ONE_CAP_WGS 6144      // one entry per wave pays up to this many workgroups (24,576 entries: the longest launch measured); longer lists keep the fixed geometry and the long road
#define FE_GL_MARGIN_PCT 125        // on a lagged length: the list of the order the launch works on is the one a later sort built
#define FE_GL_QUANTUM 128           // static_entry() keeps chunks of 64 consecutive entries on one XCD only when gridDim.x is a multiple of this

// the fixed geometry: a wave per block of the grid, at most FE_GL_FIXED_WGS workgroups -- or `cap`, the option ggrid_cap when it was set explicitly (> 0)
inline int fe_grid_launch_fixed(int blocks, int cap) {
    int g = (blocks + 3) / 4;
    if (g < 1) g = 1;
    const int c = cap > 0 ? cap : FE_GL_FIXED_WGS;
    return g < c ? g : c;
}

// Workgroups of a grid-kernel launch.  hint: the active list's length, < 0 = unknown; exact: it is the length of the very list the launch works on (else it is
// raised by margin_pct per cent); blocks: 4^3 blocks of the grid; cap: > 0 = a hard upper bound (option ggrid_cap set explicitly), 0 = none; one_cap: up to how many
// workgroups one entry per wave pays (option grid_one_cap; tuning).
// The result is a multiple of FE_GL_QUANTUM wherever the grid and the cap allow, it does not fall when the hint grows while the short road is in reach, and
// 4 x result >= hint whenever that is so (result < FE_GL_ONE_CAP_WGS and neither the cap nor the grid cut it).
inline int fe_grid_launch_wgs(long long hint, int margin_pct, bool exact, int blocks, int cap, int one_cap = FE_GL_ONE_CAP_WGS) {
    const int fixed = fe_grid_launch_fixed(blocks, cap);
    if (hint < 0) return fixed;
    if (margin_pct < 100) margin_pct = 100;
    const long long n = exact ? hint : (hint * margin_pct + 99) / 100;
    long long g = (n + 3) / 4;                                  // one entry per wave, four waves per workgroup
    if (g > one_cap) return fixed;                    // the long road either way: today's launch
    if (g < FE_GL_FLOOR_WGS) g = FE_GL_FLOOR_WGS;
    g = (g + FE_GL_QUANTUM - 1) / FE_GL_QUANTUM * FE_GL_QUANTUM;
    const long long all = blocks > 4 ? (blocks + 3) / 4 : 1;   // (no list is longer than the grid has blocks)
    if (g > all) g = all;
    if (cap > 0 && g > cap) g = cap;
    return (int)g;
}

#endif
