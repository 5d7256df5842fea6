// gemm_bf16.hip -- K2b: the vertex transforms on v_mfma_f32_32x32x16_bf16 (opt-in: dory_gemm_bf16, include/dorylus_hip.h).
//
// The operands stay fp32 in HBM and are rounded to bf16 (nearest even, v_cvt_pk_bf16_f32) in registers, between the global load
// and the LDS write; products of two bf16 values are exact in fp32 and the sums are fp32, so a product that runs here equals the
// fp32-accumulated product of its operands rounded to bf16.  One instruction multiplies 16 k where K2's (gemm.hip,
// v_mfma_f32_32x32x2_f32) multiplies 2: the 602-wide products leave the matrix unit's floor for the bytes of their operands.
//
// Geometry: K2's.  128 x BN block (BN = 128 or 64), 256 threads, each wave a 64x64 (2x2 MFMA tiles) or 32x64 (1x2) register
// tile, pick_splits's plan and splitk_reduce_kernel (gemm.hip) for the split products; the accumulator layout of the two 32x32
// instructions is the same, so the store loop is K2's.
// k-tile: GEMM_BF16_BK = 32 deep -- two 16-KB stages per 128-wide workgroup, K2's LDS footprint (64 compiles as well -- 64 KB, two workgroups
// per CU -- and has not been measured; 32 is the recorded value).
// LDS images: both bf16, [i][BK k], a row = BK/8 16-byte pieces (eight consecutive k of one i = one half-wave's fragment of the
// instruction = one ds_read_b128 per lane), the pieces of row i XOR-ed by (i >> 2) & 3 (BK = 32; (i >> 1) & 7 at 64): the 16
// lanes ds_read_b128 serves together read one logical piece of 16 consecutive rows, which the swizzle spreads over all 64 banks.
// The two kinds of source (LDS-DMA cannot round, so the tiles travel through registers):
//   row-major  elem(k,i) = p[i*ld+k]  (ah in NN; g, W in NT)   a lane takes pieces: two 16-byte loads, 4 cvt_pk, one 16-byte LDS write
//   k-major    elem(k,i) = p[k*ld+i]  (W in NN; both in TN)    wave w takes the k-group(s) 8w..8w+7: a lane loads BT/64 columns
//                                                               of eight consecutive k-rows and transposes them in registers
// Out-of-range rows (row-major) and k-rows (k-major) read zeros through the buffer resource; what a row-major row holds past
// kend -- padding, or the next split's k -- is cleared in registers in a split's last k-tile only (a uniform branch, as in K2).
// Pipeline: register-staged, the loads of tile t+1 go out before the MFMAs of tile t and are rounded and written into the other
// LDS stage after them; ONE barrier per k-tile (a stage is rewritten only after every wave has passed the barrier that follows
// its last read).
// Sum order per output element: k-tiles in order, inside a k-tile its 16-deep steps in order, inside a step the instruction's own
// fixed order -- whatever the grid; the same input gives the same bits.
// Registers (gfx950; tests/test_gemm_bf16_host.py reads them from the library), no scratch in any form:
//   128 x 64   NN 92, NT 92, TN 84 vector registers (64 accumulator registers among them)
//   128 x 128  TN 124 under amdgpu_waves_per_eu(4, 4), the occupancy of K2's 128 x 128 form; NN and NT 140 without that bound (three
//              waves per SIMD): under it they spill 3-8 registers -- 64 accumulators, 32 of raw rows in flight, 16 of fragments
// Send forms (dory_gemm_bf16_send; NN and NT only): the same main loop, then the send epilogue of gemm_bf16_tile.hpp, which keeps the
// accumulators alive through a second pass over the rows -- no scratch either (tests/test_gemm_bf16_send_host.py):
//   128 x 64   fp32 wire NN 92, NT 92; bf16 wire NN 92, NT 92
//   128 x 128  fp32 wire NN 156, NT 156; bf16 wire NN 160, NT 160 -- three waves per SIMD, as the plain NN and NT forms at 140
// The image, the loader (RegTile), the send epilogue and the launch plan live in gemm_bf16_tile.hpp, which K2c (gemm_bf16_split.hip) shares.
#include "gemm_bf16_tile.hpp"

namespace dory {

// SEND (dory_gemm_bf16_send): the same main loop, then the send epilogue of gemm_bf16_tile.hpp instead of the store loop; S16: bf16 rows
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK, bool SEND = false, bool S16 = false>
__device__ __forceinline__ void gemm_bf16_body(const GemmArgs &g, uint32_t klen, float *partial, char *smem, const GemmSend &sd = GemmSend{}) {
    static_assert(WM * WN == 4 && WN * TN * 32 == BN, "tile shape");
    static_assert(BK == 32 || BK == 64, "image geometry is written for 32- and 64-deep k-tiles");
    constexpr int BM = WM * TM * 32;
    constexpr int A_B = BM * BK * 2, STAGE = (BM + BN) * BK * 2;   // bytes
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int wm = wave / WN, wn = wave % WN;
    const uint32_t i0 = blockIdx.x * BM;
    const uint32_t j0 = blockIdx.y * BN;
    const uint32_t kbeg = blockIdx.z * klen;
    const uint32_t kend = min(g.K, kbeg + klen);
    const int fr = lane & 31, fk = lane >> 5;

    f32x16 acc[TM][TN];
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[a][b][r] = 0.f;

    RegTile<BM, A_KMAJOR, BK> ta;
    RegTile<BN, B_KMAJOR, BK> tb;
    ta.init(g.A, g.lda, g.M, i0, kbeg, kend);
    tb.init(g.B, g.ldb, g.N, j0, kbeg, kend);
    const uint32_t T = kbeg < kend ? (kend - kbeg + BK - 1) / BK : 0;
    if (T) {
        ta.load();
        tb.load();
        ta.store(smem, kend - kbeg);
        tb.store(smem + A_B, kend - kbeg);
    }
    for (uint32_t t = 0; t < T; ++t) {
        if (t + 1 < T) {   // the next tile's loads travel under this tile's MFMAs
            ta.load();
            tb.load();
        }
        // everybody's pieces of tile t are in stage t & 1, and nobody still reads the other stage (its MFMAs came before this barrier)
        __syncthreads();
        const char *As = smem + (t & 1) * STAGE;
        const char *Bs = As + A_B;
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            bf16x8 af[TM], bf[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) af[a] = *reinterpret_cast<const bf16x8 *>(As + img_off<BK>((wm * TM + a) * 32 + fr, 2 * s + fk));
#pragma unroll
            for (int b = 0; b < TN; ++b) bf[b] = *reinterpret_cast<const bf16x8 *>(Bs + img_off<BK>((wn * TN + b) * 32 + fr, 2 * s + fk));
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bf[b], acc[a][b], 0, 0, 0);
        }
        if (t + 1 < T) {
            char *nx = smem + ((t + 1) & 1) * STAGE;
            const uint32_t krem = kend - kbeg - (t + 1) * BK;
            ta.store(nx, krem);
            tb.store(nx + A_B, krem);
        }
    }

    const bool split = gridDim.z > 1;
    float *C = split ? partial + (size_t)blockIdx.z * g.M * g.ldc : g.C;
    if constexpr (SEND) {
        bf16_send_epilogue<TM, TN, S16>(g, sd, acc, C, split, i0 + wm * TM * 32, j0 + wn * TN * 32, fr, fk);
        return;
    }
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const uint32_t col = j0 + (wn * TN + b) * 32 + fr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = i0 + (wm * TM + a) * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
                if (row < g.M && col < g.N) {
                    const float v = acc[a][b][r];
                    C[(size_t)row * g.ldc + col] = v;
                    if (!split && g.epilogue == EPI_TANH) g.C2[(size_t)row * g.ldc2 + col] = dory_tanh(v);
                }
            }
        }
}

template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK>
__global__ __launch_bounds__(256) void gemm_bf16_kernel(GemmArgs g, uint32_t klen, float *partial) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * (WM * TM * 32 + BN) * BK * 2];
    gemm_bf16_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK>(g, klen, partial, smem);
}
// the 128 x 128 TN form at K2's occupancy, four waves per SIMD (NN and NT, whose row-major A tile stages 16 more registers of
// addresses and raw rows, spill 3-8 registers under that bound and run at three: file header)
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_bf16_kernel_occ4(GemmArgs g, uint32_t klen,
                                                                                                      float *partial) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * (WM * TM * 32 + BN) * BK * 2];
    gemm_bf16_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK>(g, klen, partial, smem);
}

// the send forms (dory_gemm_bf16_send): kernels of their own -- the send descriptor is their extra argument -- so that the ones above
// keep their names and code objects.  NN and NT only; no occupancy bound at either width (as the plain NN and NT forms)
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK>
__global__ __launch_bounds__(256) void gemm_bf16_send_kernel(GemmArgs g, uint32_t klen, float *partial, GemmSend sd) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * (WM * TM * 32 + BN) * BK * 2];
    gemm_bf16_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK, true, false>(g, klen, partial, smem, sd);
}
// ... and with the rows as bf16 (dory_halo_fused_pack_bf16)
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK>
__global__ __launch_bounds__(256) void gemm_bf16_send16_kernel(GemmArgs g, uint32_t klen, float *partial, GemmSend sd) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * (WM * TM * 32 + BN) * BK * 2];
    gemm_bf16_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK, true, true>(g, klen, partial, smem, sd);
}

// the kernel of a form, for launch_mfma16 (gemm_bf16_tile.hpp); TN never sends
struct K2bKernels {
    template <int BN, int WM, int WN, int TM, int TN, int BK, bool AK, bool BKM>
    void launch(dim3 grid, hipStream_t s, const GemmArgs &g, uint32_t klen, float *scratch, const GemmSend *sd) const {
        const dim3 block(256);
        if (!sd) {
            if constexpr (BN == 128 && AK)
                hipLaunchKernelGGL((gemm_bf16_kernel_occ4<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch);
            else
                hipLaunchKernelGGL((gemm_bf16_kernel<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch);
        } else if constexpr (!AK) {
            if (sd->bf16) hipLaunchKernelGGL((gemm_bf16_send16_kernel<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch, *sd);
            else hipLaunchKernelGGL((gemm_bf16_send_kernel<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch, *sd);
        }
    }
};

// K2b (kind GEMM_BF16_ROUNDED) or K2c (GEMM_BF16_SPLIT).  *taken = false and nothing launched where K2's launcher does something else
// than run a kernel, or refuses: an empty product (K == 0 is its memset) and operands off its 16-byte rule -- the caller then calls
// launch_gemm or launch_gemm_send, which behave as ever.  With sd (dory_gemm_bf16_send): *fused = the rows are in sd->buf
// (gemm_send_applies, K2's own rule); taken and not fused: the plain kernel ran and the exchange packs
hipError_t launch_gemm_bf16(const GemmArgs &g, GemmBf16Kind kind, const GemmSend *sd, float *scratch, size_t scratch_bytes, hipStream_t s,
                            bool *taken, bool *fused) {
    *fused = false;
    *taken = gemm_bf16_takes(g);
    if (!*taken) return hipSuccess;
    *fused = sd && gemm_send_applies(g, *sd);
    if (!*fused) sd = nullptr;
    if (kind == GEMM_BF16_SPLIT) return launch_gemm_bf16x3(g, scratch, scratch_bytes, s, sd);
    return launch_mfma16(K2bKernels{}, g, scratch, scratch_bytes, s, sd);
}

}  // namespace dory
