// gemm_bf16_tile.hpp -- what K2b (gemm_bf16.hip) and K2c (gemm_bf16_split.hip) share: the swizzled [i][BK k] bf16 LDS image, the
// register-staged loader of one operand's fp32 tile, the send epilogue of their send forms, and -- with K2r (gemm_bf16_resident.hip) --
// the launch plan (split count and k-length) of a 128 x BN product and the launch ladder (launch_mfma16).
// (The device text of the family stays per file: profiles/r37_gemm_family_isa.txt lists the merges that changed a kernel's instructions.)
#pragma once
#include "ctx.hpp"

namespace dory {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4v __attribute__((ext_vector_type(4)));
typedef float f32x2v __attribute__((ext_vector_type(2)));

#ifndef GEMM_BF16_BK
#define GEMM_BF16_BK 32   // k-tile depth (32 or 64)
#endif

// byte offset of the 16-byte piece q of row r in a [rows][BK] bf16 image
template <int BK>
__device__ __forceinline__ uint32_t img_off(uint32_t r, uint32_t q) {
    constexpr uint32_t PPR = BK / 8;
    const uint32_t sw = (BK == 32 ? r >> 2 : r >> 1) & (PPR - 1);
    return r * (BK * 2) + ((q ^ sw) << 4);
}

__device__ __forceinline__ bf16x8 round8(const float (&f)[8]) {
    bf16x8 v;
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = (__bf16)f[e];
    return v;
}

// One operand's tile: load() requests this thread's share of the current k-tile into registers and moves on; pieces() hands the
// eight consecutive k of every (image row, 16-byte piece) this thread holds to `emit`, store() rounds them into one LDS image.
template <int BT, bool KMAJOR, int BK>
struct RegTile {
    static constexpr int PPR = BK / 8;                              // 16-byte pieces per image row
    static constexpr int NP = KMAJOR ? PPR / 4 : BT * PPR / 256;    // row-major: pieces per thread; k-major: k-groups per wave
    static constexpr int CW = KMAJOR ? BT / 64 : 1;                 // k-major: columns per lane
    float raw[NP][8][CW];
    uint32_t voff;       // this thread's byte offset inside the current k-tile's source (constant over the k-loop)
    uint32_t pstride;    // byte distance between its consecutive pieces / k-groups
    uint32_t step;       // bytes the source advances per k-tile
    const char *base;    // source of the current k-tile
    int64_t left;        // bytes readable from base on (what lies beyond reads zeros)

    __device__ __forceinline__ void init(const float *p, uint32_t ld, uint32_t ext, uint32_t i0, uint32_t k0, uint32_t kend) {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        const uint64_t row_b = (uint64_t)ld * 4u;
        if constexpr (KMAJOR) {
            base = reinterpret_cast<const char *>(p) + (uint64_t)k0 * row_b + (uint64_t)i0 * 4u;
            voff = wave * 8u * (uint32_t)row_b + lane * (CW * 4u);
            pstride = 32u * (uint32_t)row_b;
            step = BK * (uint32_t)row_b;
            left = (int64_t)(kend - k0) * (int64_t)row_b - (int64_t)i0 * 4;
        } else {
            base = reinterpret_cast<const char *>(p) + (uint64_t)i0 * row_b + (uint64_t)k0 * 4u;
            voff = (threadIdx.x / PPR) * (uint32_t)row_b + (threadIdx.x % PPR) * 32u;
            pstride = (256u / PPR) * (uint32_t)row_b;
            step = BK * 4u;
            left = (int64_t)(ext - i0) * (int64_t)row_b - (int64_t)k0 * 4;
        }
    }
    __device__ __forceinline__ void load() {
        const uint32_t n = left <= 0 ? 0u : (left > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t)left);
        const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<char *>(base), 0, n, 0x00020000);
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) {
            const uint32_t o = pc * pstride;   // (uniform: it travels as the instruction's scalar offset, which the range check counts)
            if constexpr (KMAJOR) {
                const uint32_t row_b = step / BK;
#pragma unroll
                for (int m = 0; m < 8; ++m) {
                    if constexpr (CW == 2) {
                        const f32x2v v = __builtin_bit_cast(f32x2v, __builtin_amdgcn_raw_buffer_load_b64(rsrc, voff, o + m * row_b, 0));
                        raw[pc][m][0] = v[0];
                        raw[pc][m][CW - 1] = v[1];
                    } else {
                        raw[pc][m][0] = __builtin_bit_cast(float, __builtin_amdgcn_raw_buffer_load_b32(rsrc, voff, o + m * row_b, 0));
                    }
                }
            } else {
#pragma unroll
                for (int h = 0; h < 2; ++h) {
                    const f32x4v v = __builtin_bit_cast(f32x4v, __builtin_amdgcn_raw_buffer_load_b128(rsrc, voff + h * 16u, o, 0));
#pragma unroll
                    for (int e = 0; e < 4; ++e) raw[pc][4 * h + e][0] = v[e];
                }
            }
        }
        base += step;
        left -= step;
    }
    // krem: the k-rows of the tile that count (>= BK: all of them); emit(image row, piece, the piece's eight floats)
    template <class Emit>
    __device__ __forceinline__ void pieces(uint32_t krem, Emit &&emit) {
        const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
        if constexpr (!KMAJOR) {
            if (krem < (uint32_t)BK) {   // a split's last k-tile: a row holds padding or the next split's k past kend
                const uint32_t kq = (threadIdx.x % PPR) * 8u;
#pragma unroll
                for (int pc = 0; pc < NP; ++pc)
#pragma unroll
                    for (int e = 0; e < 8; ++e)
                        if (kq + e >= krem) raw[pc][e][0] = 0.f;
            }
        }
#pragma unroll
        for (int pc = 0; pc < NP; ++pc) {
            if constexpr (KMAJOR) {
#pragma unroll
                for (int c = 0; c < CW; ++c) {
                    float f[8];
#pragma unroll
                    for (int m = 0; m < 8; ++m) f[m] = raw[pc][m][c];
                    emit(lane * CW + c, pc * 4 + wave, f);
                }
            } else {
                float f[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) f[e] = raw[pc][e][0];
                emit(pc * (256 / PPR) + threadIdx.x / PPR, threadIdx.x % PPR, f);
            }
        }
    }
    __device__ __forceinline__ void store(char *img, uint32_t krem) {
        pieces(krem, [&](uint32_t r, uint32_t q, const float (&f)[8]) { *reinterpret_cast<bf16x8 *>(img + img_off<BK>(r, q)) = round8(f); });
    }
};

// The SEND epilogue of K2b and K2c (dory_gemm_bf16_send; the send kernels of both files end in this one copy): K2's, whose
// accumulator layout v_mfma_f32_32x32x16_bf16 shares -- lane (fr, fk) holds column fr of a 32 x 32 tile and, in register r, its row
// (r & 3) + 8 (r >> 2) + 4 fk.  row0 / col0: the first row and column of this wave's TM x TN tiles.
// Store loop: C (a split launch: this split's partial) and, with EPI_TANH, C2, exactly as the plain kernels store them; the spent
// accumulator keeps what travels -- v, tanh(v) when sd.which, zero for rows >= M and columns >= N (the padding of a padded wire row).
// Second pass (not in a split launch: the reduce kernel sends): row by row; the 32 lanes that hold a row load its slot range once and
// each slot once for all TN column tiles, and store 128 contiguous bytes per slot and tile (the slot loop inside the store loop cost
// K2 more than the pack kernel: profiles/r17_halo_fused_pack.txt).
// S16 (dory_halo_fused_pack_bf16): the rows go out as bf16, byte for byte what gather_rows_bf16_kernel leaves -- at the head of a
// row's turn, where the whole wave still walks together, a lane takes its right neighbour's column by DPP and leaves the cvt_pk dword
// of the pair in the accumulator; the even lanes store it (16 lanes x 4 bytes = the 64 contiguous bytes of a row and tile).  sd.w is
// even, so col + 1 < sd.w for an even col < sd.w.
template <int TM, int TN, bool S16>
__device__ __forceinline__ void bf16_send_epilogue(const GemmArgs &g, const GemmSend &sd, f32x16 (&acc)[TM][TN], float *C, bool split,
                                                   uint32_t row0, uint32_t col0, int fr, int fk) {
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int b = 0; b < TN; ++b) {
            const uint32_t col = col0 + b * 32 + fr;
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const uint32_t row = row0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
                float sv = 0.f;
                if (row < g.M && col < g.N) {
                    const float v = acc[a][b][r];
                    C[(size_t)row * g.ldc + col] = v;
                    sv = v;
                    if (!split && g.epilogue == EPI_TANH) {
                        const float t = dory_tanh(v);
                        g.C2[(size_t)row * g.ldc2 + col] = t;
                        if (sd.which) sv = t;
                    }
                }
                acc[a][b][r] = sv;
            }
        }
    if (split) return;
#pragma unroll
    for (int a = 0; a < TM; ++a)
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const uint32_t row = row0 + a * 32 + (r & 3) + 8 * (r >> 2) + 4 * fk;
            if constexpr (S16) {
#pragma unroll
                for (int b = 0; b < TN; ++b) acc[a][b][r] = __uint_as_float(pack_bf16x2(acc[a][b][r], lane_right(acc[a][b][r])));
            }
            if (row >= g.M) continue;
            const uint32_t s1 = sd.row_ptr[row + 1];
            for (uint32_t s = sd.row_ptr[row]; s < s1; ++s) {
                const size_t at = (size_t)sd.row_slots[s] * sd.w;   // (64-bit: a send buffer may exceed 4 GB)
#pragma unroll
                for (int b = 0; b < TN; ++b) {
                    const uint32_t col = col0 + b * 32 + fr;
                    if constexpr (S16) {
                        if (!(fr & 1) && col < sd.w)
                            *reinterpret_cast<uint32_t *>(reinterpret_cast<uint16_t *>(sd.buf) + at + col) = __float_as_uint(acc[a][b][r]);
                    } else {
                        if (col < sd.w) sd.buf[at + col] = acc[a][b][r];
                    }
                }
            }
        }
}

// The grid of a BM x BN product with BK-deep k-tiles: gemm_pick_splits's count within the scratch, then a split's k-length rounded to
// the k-tile (K2 rounds to 16) -- the rounding can only lower the split count below the one pick_splits chose, so the scratch
// gemm_scratch_bytes sized for K2 still suffices.  *klen: the k of one split; the grid's z is the split count.
inline dim3 gemm_bf16_grid(const GemmArgs &g, int BM, int BN, int BK, size_t scratch_bytes, uint32_t *klen) {
    uint32_t S = gemm_pick_splits(g.M, g.N, g.K, BM, BN);
    if (S > 1 && (size_t)S * g.M * g.ldc * sizeof(float) > scratch_bytes) {
        S = (uint32_t)(scratch_bytes / ((size_t)g.M * g.ldc * sizeof(float)));
        if (S < 2) S = 1;
    }
    *klen = (g.K + S - 1) / S;
    *klen = (*klen + BK - 1) / BK * BK;
    return dim3((g.M + BM - 1) / BM, (g.N + BN - 1) / BN, (g.K + *klen - 1) / *klen);
}

// *taken of launch_gemm_bf16: false where K2's launcher does something else than run a kernel, or refuses -- an empty product
// (K == 0 is its memset) and operands off its 16-byte rule
inline bool gemm_bf16_takes(const GemmArgs &g) {
    if (g.M == 0 || g.N == 0 || g.K == 0 || (g.ta && g.tb)) return false;
    return !((g.lda & 3u) || (g.ldb & 3u) || (reinterpret_cast<uintptr_t>(g.A) & 15u) || (reinterpret_cast<uintptr_t>(g.B) & 15u));
}

// The launch ladder of K2b, K2c and K2r.  kernels.launch<BN, WM, WN, TM, TN, BK, A_KMAJOR, B_KMAJOR>(grid, s, g, klen, scratch, sd)
// launches the file's kernel of that form -- the send form with sd (the caller has asked gemm_send_applies: NN or NT) -- and
// instantiates nothing for a form the file does not have.  A split launch is followed by K2's second-stage sum, from which a split
// send launch's rows leave.
template <int BN, int WM, int WN, int TM, int TN, int BK, class Kernels>
hipError_t launch_mfma16_bn(const Kernels &kernels, const GemmArgs &g, float *scratch, size_t scratch_bytes, hipStream_t s, const GemmSend *sd) {
    if ((g.ta && g.tb) || (sd && g.ta)) return hipErrorInvalidValue;
    uint32_t klen;
    const dim3 grid = gemm_bf16_grid(g, WM * TM * 32, BN, BK, scratch_bytes, &klen);
    if (g.ta) kernels.template launch<BN, WM, WN, TM, TN, BK, true, true>(grid, s, g, klen, scratch, sd);
    else if (g.tb) kernels.template launch<BN, WM, WN, TM, TN, BK, false, false>(grid, s, g, klen, scratch, sd);
    else kernels.template launch<BN, WM, WN, TM, TN, BK, false, true>(grid, s, g, klen, scratch, sd);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || grid.z == 1) return e;
    return sd ? launch_splitk_reduce_send(g, *sd, scratch, grid.z, s) : launch_splitk_reduce(g, scratch, grid.z, s);
}
// ... in K2's two shapes: the wide one above 64 columns
template <class Kernels>
hipError_t launch_mfma16(const Kernels &kernels, const GemmArgs &g, float *scratch, size_t scratch_bytes, hipStream_t s, const GemmSend *sd) {
    if (g.N > 64) return launch_mfma16_bn<128, 2, 2, 2, 2, GEMM_BF16_BK>(kernels, g, scratch, scratch_bytes, s, sd);
    return launch_mfma16_bn<64, 4, 1, 1, 2, GEMM_BF16_BK>(kernels, g, scratch, scratch_bytes, s, sd);
}

// K2c's side of launch_gemm_bf16 (its kernels are in gemm_bf16_split.hip's translation unit)
hipError_t launch_gemm_bf16x3(const GemmArgs &g, float *scratch, size_t scratch_bytes, hipStream_t s, const GemmSend *sd);

}  // namespace dory
