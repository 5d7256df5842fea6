// gemm_bf16_split.hip -- K2c: the vertex transforms on v_mfma_f32_32x32x16_bf16 at fp32 parity (opt-in: dory_gemm_bf16_split on top
// of dory_gemm_bf16, include/dorylus_hip.h).
//
// K2b (gemm_bf16.hip) rounds each operand to one bf16 value and so moves every product by about 2^-9.  Here each fp32 operand x is
// written as two bf16 pieces, hi = bf16(x) (nearest even) and lo = bf16(x - hi) (the subtraction is exact in fp32), which hold x to
// 2^-16, and a 16-deep step of an accumulator tile is three instructions into the same fp32 accumulator, in this fixed order, the
// small terms first:   a_lo b_hi,   a_hi b_lo,   a_hi b_hi      (a_lo b_lo, below 2^-16 of the term, is dropped).
// The operands stay fp32 in HBM -- no shadow tensor, no conversion kernel; the split happens in registers between the global load and
// the LDS write, after the k-tail of a row-major operand has been cleared (out-of-range rows and k-rows read zeros through the buffer
// resource), so both pieces are zero there.
//
// Geometry, loader, pipeline, split plan and second-stage sum: K2b's (gemm_bf16_tile.hpp; gemm_pick_splits and launch_splitk_reduce of
// gemm.hip) -- 128 x BN block (BN = 128 or 64), 256 threads, each wave 2x2 or 1x2 accumulator tiles of 32x32, register-staged prefetch
// of tile t+1 under the MFMAs of tile t, ONE barrier per k-tile; K2's store loop and tanh epilogue.
// LDS: SEPARATE images for hi and lo, per stage [A hi][A lo][B hi][B lo], each one K2b's swizzled [i][BK k] image.  A lane writes the two
// pieces of a (row, piece) at the same offset of two images (one address, the second write with an immediate offset) and reads a
// fragment's hi and lo the same way.  Bank argument: every ds_read_b128 / ds_write_b128 touches ONE image with exactly K2b's lane
// pattern, which its XOR swizzle spreads over all 64 banks, and an image's size (BT x BK x 2 bytes, a multiple of 256) leaves the bank
// of an offset unchanged -- interleaving hi and lo in one 128-byte row would need a new swizzle for no fewer instructions.
// With BK = 32: 2 stages x 2 pieces x (128 + BN) x 32 x 2 B = 64 KB at BN = 128 (two workgroups per CU in 160 KB), 48 KB at BN = 64 (three).
// Sum order per output element: k-tiles in order, inside a k-tile its 16-deep steps in order, inside a step the three instructions in
// the order above, inside an instruction its own fixed order -- whatever the grid; the same input gives the same bits.
// Registers (gfx950; tests/test_gemm_bf16_split_host.py reads them from the library), no scratch in any form; LDS bounds the occupancy
// (two waves per SIMD at BN = 128, three at 64), and amdgpu_waves_per_eu states that bound so the compiler does not trade registers
// for waves the LDS cannot hold:
//   128 x 64   NN 100, NT 98, TN 93 vector registers under amdgpu_waves_per_eu(3, 3) (32 accumulator registers among them)
//   128 x 128  NN 144, NT 142, TN 134 under amdgpu_waves_per_eu(2, 2) (64 accumulators, 32 of raw rows in flight, 32 of fragments)
// Send forms (dory_gemm_bf16_send; NN and NT only): the same main loop and occupancy bounds, then the send epilogue of
// gemm_bf16_tile.hpp -- no scratch either (tests/test_gemm_bf16_send_host.py):
//   128 x 64   fp32 wire NN 100, NT 98; bf16 wire NN 101, NT 99
//   128 x 128  fp32 wire NN 144, NT 142; bf16 wire NN 146, NT 144
#include "gemm_bf16_tile.hpp"

namespace dory {

// the two pieces of this thread's share of a tile into the hi image and the lo image that follows it `lo_off` bytes further
template <int BK, class Tile>
__device__ __forceinline__ void split_store(Tile &t, char *hi_img, uint32_t lo_off, uint32_t krem) {
    t.pieces(krem, [&](uint32_t r, uint32_t q, const float (&f)[8]) {
        bf16x8 hi, lo;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            hi[e] = (__bf16)f[e];
            lo[e] = (__bf16)(f[e] - (float)hi[e]);
        }
        char *p = hi_img + img_off<BK>(r, q);
        *reinterpret_cast<bf16x8 *>(p) = hi;
        *reinterpret_cast<bf16x8 *>(p + lo_off) = lo;
    });
}

// bytes of LDS a workgroup declares: two stages of [A hi][A lo][B hi][B lo]
template <int BM, int BN, int BK>
constexpr int bf16x3_lds() { return 2 * 2 * (BM + BN) * BK * 2; }

// SEND (dory_gemm_bf16_send): the same main loop, then the send epilogue of gemm_bf16_tile.hpp instead of the store loop; S16: bf16 rows
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK, bool SEND = false, bool S16 = false>
__device__ __forceinline__ void gemm_bf16x3_body(const GemmArgs &g, uint32_t klen, float *partial, char *smem, const GemmSend &sd = GemmSend{}) {
    static_assert(WM * WN == 4 && WN * TN * 32 == BN, "tile shape");
    static_assert(BK == 32 || BK == 64, "image geometry is written for 32- and 64-deep k-tiles");
    constexpr int BM = WM * TM * 32;
    constexpr int IMG_A = BM * BK * 2, IMG_B = BN * BK * 2, STAGE = 2 * (IMG_A + IMG_B);   // bytes
    static_assert(2 * STAGE == bf16x3_lds<BM, BN, BK>() && 2 * STAGE <= 64 * 1024, "two stages in the 64 KB a workgroup can declare");
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
        split_store<BK>(ta, smem, IMG_A, kend - kbeg);
        split_store<BK>(tb, smem + 2 * IMG_A, IMG_B, kend - kbeg);
    }
    for (uint32_t t = 0; t < T; ++t) {
        if (t + 1 < T) {   // the next tile's loads travel under this tile's MFMAs
            ta.load();
            tb.load();
        }
        // everybody's pieces of tile t are in stage t & 1, and nobody still reads the other stage (its MFMAs came before this barrier)
        __syncthreads();
        const char *As = smem + (t & 1) * STAGE;
        const char *Bs = As + 2 * IMG_A;
#pragma unroll
        for (int s = 0; s < BK / 16; ++s) {
            bf16x8 ah[TM], al[TM], bh[TN], bl[TN];
#pragma unroll
            for (int a = 0; a < TM; ++a) {
                const char *p = As + img_off<BK>((wm * TM + a) * 32 + fr, 2 * s + fk);
                ah[a] = *reinterpret_cast<const bf16x8 *>(p);
                al[a] = *reinterpret_cast<const bf16x8 *>(p + IMG_A);
            }
#pragma unroll
            for (int b = 0; b < TN; ++b) {
                const char *p = Bs + img_off<BK>((wn * TN + b) * 32 + fr, 2 * s + fk);
                bh[b] = *reinterpret_cast<const bf16x8 *>(p);
                bl[b] = *reinterpret_cast<const bf16x8 *>(p + IMG_B);
            }
            // term by term over all accumulator tiles: consecutive instructions are independent, an accumulator meets its next term
            // TM * TN instructions later
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(al[a], bh[b], acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bl[b], acc[a][b], 0, 0, 0);
#pragma unroll
            for (int a = 0; a < TM; ++a)
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ah[a], bh[b], acc[a][b], 0, 0, 0);
        }
        if (t + 1 < T) {
            char *nx = smem + ((t + 1) & 1) * STAGE;
            const uint32_t krem = kend - kbeg - (t + 1) * BK;
            split_store<BK>(ta, nx, IMG_A, krem);
            split_store<BK>(tb, nx + 2 * IMG_A, IMG_B, krem);
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
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BN == 128 ? 2 : 3, BN == 128 ? 2 : 3)))
void gemm_bf16x3_kernel(GemmArgs g, uint32_t klen, float *partial) {
    __shared__ __attribute__((aligned(1024))) char smem[bf16x3_lds<WM * TM * 32, BN, BK>()];
    gemm_bf16x3_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK>(g, klen, partial, smem);
}
// the send forms (dory_gemm_bf16_send): kernels of their own -- the send descriptor is their extra argument -- so that the one above
// keeps its name and code objects; the same occupancy bound, which the LDS sets.  NN and NT only
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BN == 128 ? 2 : 3, BN == 128 ? 2 : 3)))
void gemm_bf16x3_send_kernel(GemmArgs g, uint32_t klen, float *partial, GemmSend sd) {
    __shared__ __attribute__((aligned(1024))) char smem[bf16x3_lds<WM * TM * 32, BN, BK>()];
    gemm_bf16x3_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK, true, false>(g, klen, partial, smem, sd);
}
// ... and with the rows as bf16 (dory_halo_fused_pack_bf16)
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, bool B_KMAJOR, int BK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(BN == 128 ? 2 : 3, BN == 128 ? 2 : 3)))
void gemm_bf16x3_send16_kernel(GemmArgs g, uint32_t klen, float *partial, GemmSend sd) {
    __shared__ __attribute__((aligned(1024))) char smem[bf16x3_lds<WM * TM * 32, BN, BK>()];
    gemm_bf16x3_body<BN, WM, WN, TM, TN, A_KMAJOR, B_KMAJOR, BK, true, true>(g, klen, partial, smem, sd);
}

// the kernel of a form, for launch_mfma16 (gemm_bf16_tile.hpp); TN never sends
struct K2cKernels {
    template <int BN, int WM, int WN, int TM, int TN, int BK, bool AK, bool BKM>
    void launch(dim3 grid, hipStream_t s, const GemmArgs &g, uint32_t klen, float *scratch, const GemmSend *sd) const {
        const dim3 block(256);
        if (!sd) {
            hipLaunchKernelGGL((gemm_bf16x3_kernel<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch);
        } else if constexpr (!AK) {
            if (sd->bf16) hipLaunchKernelGGL((gemm_bf16x3_send16_kernel<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch, *sd);
            else hipLaunchKernelGGL((gemm_bf16x3_send_kernel<BN, WM, WN, TM, TN, AK, BKM, BK>), grid, block, 0, s, g, klen, scratch, *sd);
        }
    }
};

hipError_t launch_gemm_bf16x3(const GemmArgs &g, float *scratch, size_t scratch_bytes, hipStream_t s, const GemmSend *sd) {
    return launch_mfma16(K2cKernels{}, g, scratch, scratch_bytes, s, sd);
}

}  // namespace dory
