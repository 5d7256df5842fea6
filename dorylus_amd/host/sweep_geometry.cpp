// sweep_geometry.cpp -- the host arithmetic of a launch on the sweep skeleton (csrc/sweep_core.hpp: K1s in csrc/spmm.hip, the
// multi-head GAT edge passes in csrc/gat_mh_sweep.hip): the rows a lane group walks, and from them the slabs, tiles, sweeps, grid
// and gate counters of a launch.  Stated once, for the launchers (sweep_plan), for the callers that size the counters, and -- pure
// host code -- for a test without a GPU (dory_sweep_geometry).
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "../../include/dorylus_host.h"
#include "../csrc/sweep_geometry.hpp"

namespace dory {

// rows per lane group: the choice that leaves the fewest idle workgroup slots in the last sweep of a slab;
// force_r (option spmm_sweep_rows of the context; tests, experiments): 0 = pick by fill
int sweep_pick_r(uint32_t N, int group, uint32_t G, int force_r, int max_r) {
    if (force_r == 2 || force_r == 4 || force_r == 6 || force_r == 8 || (force_r == 10 && group == 32 && max_r >= 10) ||
        ((force_r == 3 || force_r == 5) && group == 16))
        return force_r;
    const uint32_t rpx = (N + 7) / 8;
    int best = 8;
    double best_fill = 0;
    for (int R : {10, 8, 6, 4, 2}) {            // few rows per group: small partitions (one of 8 ranks) still fill every CU
        if ((group == 16 && R == 10) || R > max_r) continue;   // 16-lane groups stage twice the entries per lane: 10 rows would spill
        const uint32_t RW = (uint32_t)(SWEEP_NT / group) * R;
        const uint32_t tiles = (rpx + RW - 1) / RW;
        const uint32_t spp = (tiles + G - 1) / G;
        const double fill = (double)rpx / ((double)spp * G * RW);
        if (fill > best_fill + 0.02) { best_fill = fill; best = R; }
    }
    return best;
}

// rows per lane group of a K1s launch on `group` lanes: what the layout (rows_per_group, npos) was dealt for, unless forced
// (force_r: the option) or not instantiated for the lane-group width
int sweep_rows(uint32_t rows_per_group, uint32_t npos, int group, uint32_t G, int force_r) {
    const int forced = sweep_pick_r(0, group, G, force_r, 10);      // (returns the forced value whatever N when one is valid)
    if (force_r && forced == force_r) return forced;
    // (16-lane groups stage twice the entries per lane: eight rows spill two registers into the chain LDS -> gathers -> sums;
    // a spilling variant is not launched unless an option forces it -- tests/test_kernel_resources.py)
    // 16-lane launches (64-float rows) have twice the lane groups per workgroup: half the layout's rows per group walks the
    // rows per workgroup and step the layout was dealt for, and leaves registers for the loader wave (round 5: the 64-float
    // aggregations of the GAT prototype 2.00 -> see DESIGN; 6 rows without the loader was the round-4 form)
    if (rows_per_group && group == 16) return std::max<int>(2, (int)rows_per_group / 2);
    if (rows_per_group && group == 32) return (int)rows_per_group;
    return sweep_pick_r(npos, group, G, 0, 10);
}

// the row counts of 16-lane groups that K1s's wide form (eight features per lane: spmm_sweep_bf16x8_kernel) is instantiated for
// (2 .. 5: a forced 6 or 8 keeps the narrow form)
bool sweep_wide_rows_ok(int R) { return R >= 2 && R <= 5; }

// A launch that walks R rows per lane group over npos positions, on rows of ld floats, G workgroups per sweep and XCD.
// wide: 16-lane groups on chunks of eight features, whatever `group`.
SweepGeometry sweep_geometry(uint32_t npos, uint32_t ld, int group, int R, bool wide, uint32_t G) {
    if (wide) group = 16;
    const uint32_t RW = (uint32_t)(SWEEP_NT / group) * R;   // rows per workgroup
    SweepGeometry g;
    g.slabs = ((ld >> (wide ? 3 : 2)) + group - 1) / group;
    g.rpx = ((npos + 7) / 8 + R - 1) / R * R;
    g.tiles_x = (g.rpx + RW - 1) / RW;
    g.spp = (g.tiles_x + G - 1) / G;
    g.nsweeps = g.slabs * g.spp;
    g.grid_x = 8u * g.nsweeps * G;
    g.block_words = 8u * g.nsweeps * 32u;
    return g;
}

// bytes of gate counters a launch of geometry g over nblocks source blocks clears (+ 1: the "gates off" word)
size_t sweep_counter_bytes(const SweepGeometry &g, uint32_t nblocks) {
    return ((size_t)g.block_words * nblocks + 1) * sizeof(uint32_t);
}

// ... and what any launch of that shape over nblocks blocks may need: a launch may leave up to 8 of more than 12 CUs per XCD
// to concurrent kernels (SweepPart::reserve), and nsweeps does not grow with G
size_t sweep_counter_bound(uint32_t npos, uint32_t ld, int group, int R, bool wide, uint32_t G, uint32_t nblocks) {
    return sweep_counter_bytes(sweep_geometry(npos, ld, group, R, wide, G > 12 ? G - 8 : G), nblocks);
}

}  // namespace dory

extern "C" int dory_sweep_geometry(uint32_t positions, uint32_t ld, int group, int rows, int wide, uint32_t cus, uint32_t nblocks,
                                   uint32_t layout_rows, int rows_option, uint64_t *out) {
    if (!out || (group != 16 && group != 32) || rows < 1 || cus < 1 || cus > 32 || (ld & (wide ? 7u : 3u))) return 1;
    const dory::SweepGeometry g = dory::sweep_geometry(positions, ld, group, rows, wide != 0, cus);
    const uint64_t v[] = {g.slabs, g.rpx, g.tiles_x, g.spp, g.nsweeps, g.grid_x, g.block_words,
                          dory::sweep_counter_bytes(g, nblocks) / sizeof(uint32_t),
                          dory::sweep_counter_bound(positions, ld, group, rows, wide != 0, cus, nblocks) / sizeof(uint32_t),
                          (uint64_t)dory::sweep_rows(layout_rows, positions, wide ? 16 : group, cus, rows_option),
                          (uint64_t)dory::sweep_wide_rows_ok(dory::sweep_rows(layout_rows, positions, 16, cus, rows_option))};
    std::copy(v, v + sizeof(v) / sizeof(v[0]), out);
    return 0;
}
