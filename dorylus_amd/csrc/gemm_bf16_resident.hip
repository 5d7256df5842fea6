// gemm_bf16_resident.hip -- K2r: K2b (gemm_bf16.hip) with its A operand read from a resident bf16 copy (opt-in:
// dory_gemm_bf16_resident, include/dorylus_hip.h).
//
// The A operand of the layer-0 products (x, fg@0, a kept ah@0; h@0 of the GAT models) is the same matrix every epoch.  K2b reads it
// as fp32 and rounds it in registers, twice per epoch; here it is rounded once (gemm_resident_rows_kernel, nearest even -- the cast
// of K2b's round8 and of the shadow rows) into rows x ldr bf16, ldr = cols rounded up to 32 with zeros in [cols, ldr), and the
// products read that: half the bytes of the operand, and every 32-deep k-tile of a row one whole 16-byte-aligned 64-byte run.
// The other operand (W, or the gradient of TN) stays fp32 and travels by K2b's RegTile.
//
// Geometry, split plan, LDS image (img_off<32>), fragment reads, MFMA order and store loop are K2b's, so a product here gives
// K2b's bits: k-tiles in order, inside a k-tile its 16-deep steps in order, inside a step the instruction's own order.
//
// NN (A row-major, [i][k]): the A tile travels global -> LDS by `buffer_load_dwordx4 ... lds`, no VGPRs.  A stage's 128 x 32 bf16
// is 8 KB = eight 1-KB pieces of 16 rows, two per wave.  The DMA writes lane-linear, so the image's swizzle is on the source side:
// lane l of a piece writes row r = l >> 2, physical piece l & 3, and fetches logical piece (l & 3) ^ ((r >> 2) & 3) of that row.
// Rows past M read zeros through the resource's byte count; the k-tail is the copy's zero padding (a split is a whole number of
// k-tiles), so there is no tail-clearing branch for A.  Per k-tile: barrier, W's loads of tile t+1, the 16-deep steps of tile t
// with the DMA of tile t+1 behind the LAST step's fragment reads and ahead of its MFMAs (hipcc orders an LDS read behind a pending
// LDS-DMA with vmcnt(0), gemm.hip), W's LDS write, then vmcnt(0) before the next barrier publishes the stage.
// TN (A k-major, [k][i], k the vertex index): the matrix unit wants eight consecutive k per lane, the copy has consecutive i, so the
// tile still transposes in registers -- K2b's k-major scheme (wave w owns the k-rows 8w..8w+7) on bf16: a lane loads ONE dword (two
// adjacent columns) of each of the eight k-rows and splits them into the two columns' 16-byte pieces; half the load instructions
// and bytes of K2b's arm and no conversion.  k-rows past the split's end read zeros through the resource.  Pipeline: K2b's.
// Registers (gfx950; tests/test_gemm_bf16_resident_host.py reads them from the library), no scratch in any form:
//   128 x 64   NN 84, TN 76 vector registers
//   128 x 128  NN 117, TN 116, both under amdgpu_waves_per_eu(4, 4): the NN form, which K2b runs at 140 registers and three waves
//              per SIMD, fits K2's four (with every step's fragments read ahead of the DMA it needs 129 under that bound; the form
//              without the bound was not built)
#include "gemm_bf16_tile.hpp"

namespace dory {

// rows x ldr bf16 from rows x ld fp32: two elements per thread, zeros in [cols, ldr)
__global__ __launch_bounds__(256) void gemm_resident_rows_kernel(const float *x, uint32_t ld, uint32_t cols, uint32_t *y, uint32_t pairs_per_row,
                                                                 uint64_t n) {
    const uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const uint64_t r = i / pairs_per_row;
    const uint32_t k = (uint32_t)(i - r * pairs_per_row) * 2u;
    const float *p = x + r * ld;
    y[i] = pack_bf16x2(k < cols ? p[k] : 0.f, k + 1 < cols ? p[k + 1] : 0.f);
}

hipError_t launch_gemm_resident_rows(const float *x, uint32_t ld, uint64_t rows, uint32_t cols, uint16_t *y, uint32_t ldr, hipStream_t s) {
    const uint64_t n = rows * (ldr / 2);
    if (!n) return hipSuccess;
    hipLaunchKernelGGL(gemm_resident_rows_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, x, ld, cols, reinterpret_cast<uint32_t *>(y),
                       ldr / 2, n);
    return hipGetLastError();
}

// The row-major A tile of NN: 128 x BK bf16 of the resident copy into the swizzled image by LDS-DMA (DmaTile's row-major arm of
// gemm.hip on 2-byte elements)
template <int BM, int BK>
struct ResDmaTile {
    static_assert(BM == 128 && BK == 32, "a piece is 16 rows of 64 bytes");
    static constexpr int PIECES = BM * BK * 2 / 1024 / 4;   // 1-KB pieces per wave (4 waves)
    uint32_t voff;       // this lane's byte offset inside a piece's source (constant over the k-loop)
    uint32_t pstride;    // byte distance between this wave's consecutive pieces
    const char *base;    // source of the current k-tile
    int64_t left;        // bytes readable from base on (rows beyond it read zeros)

    __device__ __forceinline__ void init(const uint16_t *p, uint32_t ldr, uint32_t rows, uint32_t i0, uint32_t k0) {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint64_t row_b = (uint64_t)ldr * 2u;
        const uint32_t r = wave * PIECES * 16u + (lane >> 2);
        const uint32_t q = (lane & 3u) ^ ((r >> 2) & 3u);
        base = reinterpret_cast<const char *>(p) + (uint64_t)i0 * row_b + (uint64_t)k0 * 2u;
        voff = r * (uint32_t)row_b + q * 16u;
        pstride = 16u * (uint32_t)row_b;
        left = (int64_t)(rows - i0) * (int64_t)row_b - (int64_t)k0 * 2;
    }
    // issue this wave's pieces of the current k-tile into `img`, then move on to the next k-tile
    __device__ __forceinline__ void issue(char *img) {
        const uint32_t wave = threadIdx.x >> 6;
        const uint32_t n = left <= 0 ? 0u : (left > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)left);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, n, 0x00020000);
        typedef __attribute__((address_space(3))) void *lptr_t;
#pragma unroll
        for (int pc = 0; pc < PIECES; ++pc)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsrc, (lptr_t)(img + (wave * PIECES + pc) * 1024), 16, voff, pc * pstride, 0, 0);
        base += BK * 2;
        left -= BK * 2;
    }
};

// The k-major A tile of TN: BK k-rows x 128 columns of the resident copy, transposed in registers (RegTile's k-major arm on bf16)
template <int BM, int BK>
struct ResKTile {
    static_assert(BM == 128 && BK == 32, "a lane holds two columns, a wave one k-group");
    uint32_t raw[8];     // the dword (columns 2 lane, 2 lane + 1) of this wave's eight k-rows
    uint32_t voff, row_b;
    const char *base;
    int64_t left;

    __device__ __forceinline__ void init(const uint16_t *p, uint32_t ldr, uint32_t i0, uint32_t k0, uint32_t kend) {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        row_b = ldr * 2u;
        base = reinterpret_cast<const char *>(p) + (uint64_t)k0 * row_b + (uint64_t)i0 * 2u;
        voff = wave * 8u * row_b + lane * 4u;
        left = (int64_t)(kend - k0) * (int64_t)row_b - (int64_t)i0 * 2;
    }
    __device__ __forceinline__ void load() {
        const uint32_t n = left <= 0 ? 0u : (left > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)left);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, n, 0x00020000);
#pragma unroll
        for (int m = 0; m < 8; ++m) raw[m] = __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, m * row_b, 0);
        base += (uint64_t)BK * row_b;
        left -= (int64_t)BK * row_b;
    }
    // column 2 lane takes the low halves of the eight dwords, column 2 lane + 1 the high ones: piece `wave` of their image rows
    __device__ __forceinline__ void store(char *img) const {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        uint4 lo, hi;
        lo.x = (raw[0] & 0xFFFFu) | (raw[1] << 16); hi.x = (raw[0] >> 16) | (raw[1] & 0xFFFF0000u);
        lo.y = (raw[2] & 0xFFFFu) | (raw[3] << 16); hi.y = (raw[2] >> 16) | (raw[3] & 0xFFFF0000u);
        lo.z = (raw[4] & 0xFFFFu) | (raw[5] << 16); hi.z = (raw[4] >> 16) | (raw[5] & 0xFFFF0000u);
        lo.w = (raw[6] & 0xFFFFu) | (raw[7] << 16); hi.w = (raw[6] >> 16) | (raw[7] & 0xFFFF0000u);
        *reinterpret_cast<uint4 *>(img + img_off<BK>(2 * lane, wave)) = lo;
        *reinterpret_cast<uint4 *>(img + img_off<BK>(2 * lane + 1, wave)) = hi;
    }
};

// B (k-major, fp32) is K2b's RegTile in both forms
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, int BK>
__device__ __forceinline__ void gemm_res_body(const GemmArgs &g, const uint16_t *R, uint32_t ldr, uint32_t klen, float *partial, char *smem) {
    static_assert(WM * WN == 4 && WN * TN * 32 == BN, "tile shape");
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

    RegTile<BN, true, BK> tb;
    tb.init(g.B, g.ldb, g.N, j0, kbeg, kend);
    const uint32_t T = kbeg < kend ? (kend - kbeg + BK - 1) / BK : 0;
    if constexpr (A_KMAJOR) {
        ResKTile<BM, BK> ta;
        ta.init(R, ldr, i0, kbeg, kend);
        if (T) {
            ta.load();
            tb.load();
            ta.store(smem);
            tb.store(smem + A_B, kend - kbeg);
        }
        for (uint32_t t = 0; t < T; ++t) {
            if (t + 1 < T) {   // the next tile's loads travel under this tile's MFMAs
                ta.load();
                tb.load();
            }
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
                ta.store(nx);
                tb.store(nx + A_B, kend - kbeg - (t + 1) * BK);
            }
        }
    } else {
        ResDmaTile<BM, BK> ta;
        ta.init(R, ldr, g.M, i0, kbeg);
        if (T) {
            ta.issue(smem);
            tb.load();
            tb.store(smem + A_B, kend - kbeg);
        }
        for (uint32_t t = 0; t < T; ++t) {
            // this wave's DMA pieces of tile t have landed; past the barrier everybody's have, W's rows are written, and nobody still
            // reads the other stage
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
            if (t + 1 < T) tb.load();
            const char *As = smem + (t & 1) * STAGE;
            const char *Bs = As + A_B;
            char *nx = smem + ((t + 1) & 1) * STAGE;
#pragma unroll
            for (int s = 0; s < BK / 16; ++s) {
                bf16x8 af[TM], bf[TN];
#pragma unroll
                for (int a = 0; a < TM; ++a) af[a] = *reinterpret_cast<const bf16x8 *>(As + img_off<BK>((wm * TM + a) * 32 + fr, 2 * s + fk));
#pragma unroll
                for (int b = 0; b < TN; ++b) bf[b] = *reinterpret_cast<const bf16x8 *>(Bs + img_off<BK>((wn * TN + b) * 32 + fr, 2 * s + fk));
                // (after the tile's last fragment reads: file header -- with every step's fragments read first the 128 x 128 form
                // needs 129 registers under four waves per SIMD)
                if (s == BK / 16 - 1 && t + 1 < T) ta.issue(nx);
#pragma unroll
                for (int a = 0; a < TM; ++a)
#pragma unroll
                    for (int b = 0; b < TN; ++b) acc[a][b] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(af[a], bf[b], acc[a][b], 0, 0, 0);
            }
            if (t + 1 < T) tb.store(nx + A_B, kend - kbeg - (t + 1) * BK);
        }
    }

    const bool split = gridDim.z > 1;
    float *C = split ? partial + (size_t)blockIdx.z * g.M * g.ldc : g.C;
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

template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, int BK>
__global__ __launch_bounds__(256) void gemm_bf16_resident_kernel(GemmArgs g, const uint16_t *R, uint32_t ldr, uint32_t klen, float *partial) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * (WM * TM * 32 + BN) * BK * 2];
    gemm_res_body<BN, WM, WN, TM, TN, A_KMAJOR, BK>(g, R, ldr, klen, partial, smem);
}
// the 128 x 128 forms at K2's occupancy, four waves per SIMD
template <int BN, int WM, int WN, int TM, int TN, bool A_KMAJOR, int BK>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4, 4))) void gemm_bf16_resident_kernel_occ4(GemmArgs g, const uint16_t *R,
                                                                                                               uint32_t ldr, uint32_t klen,
                                                                                                               float *partial) {
    __shared__ __attribute__((aligned(1024))) char smem[2 * (WM * TM * 32 + BN) * BK * 2];
    gemm_res_body<BN, WM, WN, TM, TN, A_KMAJOR, BK>(g, R, ldr, klen, partial, smem);
}

// the kernel of a form, for launch_mfma16 (gemm_bf16_tile.hpp)
struct K2rKernels {
    const uint16_t *R;
    uint32_t ldr;
    template <int BN, int WM, int WN, int TM, int TN, int BK, bool AK, bool BKM>
    void launch(dim3 grid, hipStream_t s, const GemmArgs &g, uint32_t klen, float *scratch, const GemmSend *) const {
        const dim3 block(256);
        if constexpr (BKM) {   // (NN and TN only: gemm_bf16_resident_takes)
            if constexpr (BN == 128)
                hipLaunchKernelGGL((gemm_bf16_resident_kernel_occ4<BN, WM, WN, TM, TN, AK, BK>), grid, block, 0, s, g, R, ldr, klen, scratch);
            else
                hipLaunchKernelGGL((gemm_bf16_resident_kernel<BN, WM, WN, TM, TN, AK, BK>), grid, block, 0, s, g, R, ldr, klen, scratch);
        }
    }
};

bool gemm_bf16_resident_takes(const GemmArgs &g) { return !g.tb && gemm_bf16_takes(g); }

// R: the resident copy of the tensor behind g.A, rows x ldr bf16 (ldr a multiple of 32, zeros past the tensor's columns).  NN reads
// g.M rows of g.K <= ldr columns, TN g.K rows of g.M columns; the caller has asked gemm_bf16_resident_takes(g).
hipError_t launch_gemm_bf16_resident(const GemmArgs &g, const uint16_t *R, uint32_t ldr, float *scratch, size_t scratch_bytes, hipStream_t s) {
    if (!gemm_bf16_resident_takes(g) || !R || (ldr & 31u) || (!g.ta && g.K > ldr)) return hipErrorInvalidValue;
    return launch_mfma16(K2rKernels{R, ldr}, g, scratch, scratch_bytes, s, nullptr);   // K2b's plan: the same splits, the same bits
}

}  // namespace dory
