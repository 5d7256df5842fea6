// sweep_geometry.hpp -- what host/sweep_geometry.cpp (pure host code) and the sweep skeleton (sweep_core.hpp) must agree on:
// the threads of a sweep workgroup and the record of a launch's geometry.  No HIP in here.
#ifndef DORY_SWEEP_GEOMETRY_HPP
#define DORY_SWEEP_GEOMETRY_HPP
#include <cstdint>

namespace dory {

constexpr int SWEEP_NT = 1024;

// one launch on rows of ld floats over the positions of a sweep layout (host/sweep_geometry.cpp: sweep_geometry)
struct SweepGeometry {
    uint32_t slabs;        // feature slabs of a row: `group` lanes of four floats (wide: sixteen lanes of eight)
    uint32_t rpx;          // destination rows per XCD: whole lane groups
    uint32_t tiles_x;      // workgroups per XCD and slab
    uint32_t spp;          // sweeps per slab: ceil(tiles_x / G)
    uint32_t nsweeps;      // slabs * spp
    uint32_t grid_x;       // workgroups of the launch
    uint32_t block_words;  // gate counter words per source block: [8][nsweeps][32]
};

}  // namespace dory
#endif
