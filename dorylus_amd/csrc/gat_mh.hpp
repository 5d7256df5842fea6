// gat_mh.hpp -- shared by gat_mh.hip (row-wise kernels, launchers), gat_mh_blocked.hip (source-blocked kernels) and
// gat_mh_sweep.hip (the edge passes on the sweep skeleton)
#ifndef DORY_GAT_MH_HPP
#define DORY_GAT_MH_HPP
#include "ctx.hpp"
#include "gat_mh_shapes.hpp"   // gatmh_shape_ok and the row-gather family's shape rules (host code asks them too)

namespace dory {

constexpr float GATMH_SLOPE = 0.2f;
constexpr int GATMH_MAXC = 4;   // K*D <= 256 (row-wise kernels are instantiated for 1, 2 or 4 chunks of 64 floats)
static_assert(64 * GATMH_MAXC == 256, "gatmh_shape_ok (gat_mh_shapes.hpp) states the bound as 256");

__device__ __forceinline__ float lrelu02(float x) { return x > 0.f ? x : GATMH_SLOPE * x; }
// one DPP move inside the VALU (CTRL: a quad_perm, row_half_mirror 0x141, row_mirror 0x140)
template <int CTRL>
__device__ __forceinline__ float dpp_mov(float v) {
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), CTRL, 0xF, 0xF, true));
}

struct GatMhArgs {
    uint32_t N, K, D, ld /*of z, o, do, dz*/, ldk /*of el, er, m, den, t, del, der*/;
    const uint64_t *ptr;   // CSC (forward / dst pass) or CSR (src pass)
    const uint32_t *idx;
};

}  // namespace dory
#endif
