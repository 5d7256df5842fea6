// gat_mh_shapes.hpp -- the shape rules of the multi-head GAT's kernels that host code without a device asks too (plain C++, no HIP):
// which head shapes the model allows, which rows the row-gather family (gat_mh_rows.hip) covers, and where its bf16 form has a wide
// (16-byte) sibling (dory_gatmh_row_gather_bf16_wide; include/dorylus_host.h: dory_gatmh_row_gather_bf16_wide_form).
#ifndef DORY_GAT_MH_SHAPES_HPP
#define DORY_GAT_MH_SHAPES_HPP
#include <cstdint>

namespace dory {

// K heads of D features fit the kernels: K*D <= 256, D a power of two <= 64 unless there is a single head
inline bool gatmh_shape_ok(uint32_t K, uint32_t D) {
    if (K == 0 || D == 0 || K > 64 || (uint64_t)K * D > 256) return false;
    if (K == 1) return true;
    return (D & (D - 1)) == 0 && D <= 64;   // per-head reductions are xor-shuffles inside D lanes
}
// the rows the row-gather family covers: a shape of the model on rows float4s tile, at most 256 floats
inline bool gatmh_rows_shape_ok(uint32_t K, uint32_t D, uint32_t ld) {
    return gatmh_shape_ok(K, D) && !(ld & 3) && ld != 0 && ld <= 256 && K * D <= ld;
}
// The wide bf16 form of the row-gather family: a lane keeps EIGHT consecutive features (one 16-byte load of eight bf16 per edge), so a
// row takes half the narrow form's lanes.  Taken where the family covers the shape, rows are 16-byte tiled and at least 64 floats (a
// 32-float row would be four lanes), and a lane's eight features lie in one head (a single head, or D % 8 == 0: no wide counterpart of
// two or four heads per float4).  lanes_row: 8 / 16 / 32 by ld / 8; lanes_head: the lanes a head's dot products are reduced over (the
// group for a single head, else D / 8); scores_from_row: the sources' scores come from the gathered row exactly where the narrow
// form's do (ld / 4 a power of two), else el / fg_el are gathered.
inline bool gatmh_rows8_form(uint32_t K, uint32_t D, uint32_t ld, uint32_t *lanes_row, uint32_t *lanes_head, int *scores_from_row) {
    if (!gatmh_rows_shape_ok(K, D, ld) || ld < 64 || (ld & 7)) return false;
    if (K != 1 && (D & 7)) return false;
    const uint32_t n8 = ld >> 3, n4 = ld >> 2;
    *lanes_row = n8 <= 8 ? 8 : n8 <= 16 ? 16 : 32;
    *lanes_head = K == 1 ? *lanes_row : D >> 3;
    *scores_from_row = (n4 & (n4 - 1)) == 0;
    return true;
}

}  // namespace dory
#endif
