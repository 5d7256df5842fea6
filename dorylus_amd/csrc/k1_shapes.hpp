// k1_shapes.hpp -- the form rule of K1's wide bf16 row gather (spmm.hip: spmm_rows_bf16x8_kernel; dory_k1_bf16_wide) as launch_spmm
// applies it, for host code without a device too (plain C++, no HIP; include/dorylus_hip.h: dory_k1_bf16_wide_form).
#ifndef DORY_K1_SHAPES_HPP
#define DORY_K1_SHAPES_HPP
#include <cstdint>

namespace dory {

// The lanes x chunks that rows of 32 < ceil(width / 8) <= 48 sixteen-byte chunks run on -- Amazon's 300 floats, ld 320: 40 chunks.
// 0: (64, 1), 24 of 64 lanes idle on ld 320.  1: (16, 3), 8 of 48 idle, four rows per wave at three times the accumulators -- built only
// where this is 1 (the measurement of tools/k1_bf16_wide_rate.py), since the resource test admits exactly the forms the rule selects.
#ifndef DORY_K1_WIDE_CH48_16X3
#define DORY_K1_WIDE_CH48_16X3 0
#endif

// The wide form of K1 on bf16 rows: a lane keeps EIGHT consecutive features per chunk (one 16-byte load of eight bf16 per edge).  `slab`
// is option spmm_slab (floats per feature slab, 0 = none); the width of one block pass is launch_spmm's: ld, or the slab where it is
// narrower.  No form -- the narrow one runs -- where ld < 64 (a 32-float row is four chunks, fewer than the smallest lane group), where
// ld is no multiple of 8, or where a pass is under 64 floats wide.  Otherwise the narrow table's shape by ch8 = ceil(width / 8); rows
// wider than 64 x 3 chunks (1536 floats) take gridDim.y slabs of the (64, 3) form: wide has no 4-chunk instantiation.
inline bool k1_rows8_form(uint32_t ld, uint32_t slab, uint32_t *lanes, uint32_t *chunks) {
    if (ld < 64 || (ld & 7)) return false;
    uint32_t width = ld;
    if (slab > 0 && slab < width) width = slab;
    if (width < 64) return false;
    const uint32_t ch8 = (width + 7) / 8;
    uint32_t g, k;
    if (ch8 <= 8) { g = 8; k = 1; }
    else if (ch8 <= 16) { g = 16; k = 1; }
    else if (ch8 <= 32) { g = 32; k = 1; }
    else if (DORY_K1_WIDE_CH48_16X3 && ch8 <= 48) { g = 16; k = 3; }
    else if (ch8 <= 64) { g = 64; k = 1; }
    else if (ch8 <= 96) { g = 32; k = 3; }
    else if (ch8 <= 128) { g = 64; k = 2; }
    else { g = 64; k = 3; }
    *lanes = g;
    *chunks = k;
    return true;
}

}  // namespace dory
#endif
