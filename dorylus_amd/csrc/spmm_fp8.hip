// spmm_fp8.hip -- K1, the row gather (spmm.hip), on fp8 rows: dory_k1_fp8_gather (include/dorylus_hip.h).
//
// The rows an aggregation reads -- self row, local and ghost rows -- are rounded to OCP E4M3 with ONE power-of-two scale per row
// (fp8_rows_kernel; the definition is dory_k1_fp8_rows, host/k1_fp8.cpp) into a shadow buffer [N local rows ; ghost rows] of ld BYTES
// per row and one biased exponent byte per row.  Edge values, norm, the sums and `out` stay fp32, the sums in K1's order: per output
// element the same fmaf chain in edge order from the same start (zero, the self term, or the first pass's sum) as spmm_rows_kernel on
// the dequantised rows -- same bits.
//
//   * a source row's bytes are a quarter of its fp32 row: a 128-float row is ONE 128-byte line.  A lane keeps SIXTEEN consecutive
//     features per chunk (one 16-byte load per lane, edge and chunk; four float4 sums), or eight on rows of 64 / 96 floats
//     (k1_shapes.hpp: k1_fp8_form); four edges are in flight per lane group as raw bytes and widened as they are summed.
//   * the shadow rows are one array, so a source id (ghost ids are N + k) addresses row and exponent directly: K1's ghost select
//     is the index itself.  The lane that loads an entry's idx / val loads the source's exponent byte and broadcasts 2^e with them.
//   * dequantisation is v_cvt_scalef32_pk_f32_fp8: two E4M3 -> two fp32 times 2^e in one instruction, exact (the exponent range of
//     fp8_rows_kernel keeps every q * 2^e a normal fp32 or zero).  Folding 2^e into the edge weight instead would round where
//     val * 2^e leaves the normal range, and break the bit contract; DORY_K1_FP8_SCALE_CVT = 0 builds v_cvt_pk_f32_fp8 + v_mul_f32
//     (the same values, two more instructions per four features).
//   * no LDS, no atomics, no waits in the gather; the long-row kernels are spmm_longrow_body's (4 waves over a chunk, wave partials
//     added in wave order through LDS, chunk sums added in chunk order).
#include "k1_shapes.hpp"
#include "spmm_common.hpp"

#ifndef DORY_K1_FP8_SCALE_CVT
#define DORY_K1_FP8_SCALE_CVT 1
#endif

namespace dory {

typedef float v2f __attribute__((ext_vector_type(2)));
template <int NW> using Words = uint32_t __attribute__((ext_vector_type(NW)));   // NW x four E4M3 as loaded

// the exponent byte of a row -> 2^e as fp32 (the byte IS the fp32 exponent field: 10 .. 246, never 0 or 255)
__device__ __forceinline__ float fp8_scale(uint32_t ebyte) { return __uint_as_float(ebyte << 23); }

// four E4M3 (one word, element 0 in the low byte) times `scale`, exactly
__device__ __forceinline__ float4 fp8x4_to_float4(uint32_t w, float scale) {
#if DORY_K1_FP8_SCALE_CVT
    const v2f lo = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, scale, false);
    const v2f hi = __builtin_amdgcn_cvt_scalef32_pk_f32_fp8(w, scale, true);
    return make_float4(lo.x, lo.y, hi.x, hi.y);
#else
    const v2f lo = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, false);
    const v2f hi = __builtin_amdgcn_cvt_pk_f32_fp8((int)w, true);
    return make_float4(lo.x * scale, lo.y * scale, hi.x * scale, hi.y * scale);
#endif
}

// ---- the conversion ----------------------------------------------------------------------------------------------------------
// byte = clamp(exponent field of the row's absolute maximum - 7, 10, 246), i.e. e = floor(log2 max) - 7 in [-117, 119]; 127 (e = 0)
// for an all-zero row.  Returns the byte; *inv = 2^-e.
__device__ __forceinline__ uint32_t fp8_row_exponent(float amax, float *inv) {
    int b = (int)(__float_as_uint(amax) >> 23) - 7;
    b = amax == 0.f ? 127 : (b < 10 ? 10 : (b > 246 ? 246 : b));
    *inv = __uint_as_float((uint32_t)(254 - b) << 23);
    return (uint32_t)b;
}
__device__ __forceinline__ float amax4(const float4 &x, float m) {
    return fmaxf(fmaxf(fmaxf(fabsf(x.x), fabsf(x.y)), fmaxf(fabsf(x.z), fabsf(x.w))), m);
}
// four floats scaled by 2^-e (exact), held to E4M3's +-448 (only a maximum of 2^127 or more gets there: e stops at 119), rounded to
// nearest even by the hardware conversion, subnormals included
__device__ __forceinline__ uint32_t fp8_pack4(const float4 &x, float inv) {
    const float a = fminf(fmaxf(x.x * inv, -448.f), 448.f), b = fminf(fmaxf(x.y * inv, -448.f), 448.f);
    const float c = fminf(fmaxf(x.z * inv, -448.f), 448.f), d = fminf(fmaxf(x.w * inv, -448.f), 448.f);
    int w = __builtin_amdgcn_cvt_pk_fp8_f32(a, b, 0, false);
    w = __builtin_amdgcn_cvt_pk_fp8_f32(c, d, w, true);
    return (uint32_t)w;
}
template <int GROUP>
__device__ __forceinline__ float group_max(float m) {
#pragma unroll
    for (int o = GROUP / 2; o > 0; o >>= 1) m = fmaxf(m, __shfl_xor(m, o, GROUP));   // butterfly: every lane of the group ends with the maximum
    return m;
}

// One lane group per row, V consecutive float4 per lane: the row is read once and kept in registers; 4 V bytes stored per lane.
// Rows of up to GROUP * V * 4 floats (launch_fp8_rows picks; lanes past the row hold zeros and store nothing).
template <int GROUP, int V>
__global__ __launch_bounds__(256) void fp8_rows_kernel(const float *x, uint8_t *q, uint8_t *e, uint64_t rows, uint32_t ld) {
    constexpr int RPW = 64 / GROUP, RPB = 4 * RPW;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t li = lane % GROUP, gi = lane / GROUP;
    const uint64_t row = (uint64_t)blockIdx.x * RPB + wave * RPW + gi;
    const bool act = row < rows && li * (4 * V) < ld;
    float4 v[V];
    float m = 0.f;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        v[i] = act ? reinterpret_cast<const float4 *>(x)[row * (ld >> 2) + li * V + i] : make_float4(0.f, 0.f, 0.f, 0.f);
        m = amax4(v[i], m);
    }
    m = group_max<GROUP>(m);
    float inv;
    const uint32_t eb = fp8_row_exponent(m, &inv);
    if (!act) return;
    Words<V> w;
#pragma unroll
    for (int i = 0; i < V; ++i) {
        if constexpr (V == 1) w = fp8_pack4(v[i], inv);
        else w[i] = fp8_pack4(v[i], inv);
    }
    *reinterpret_cast<Words<V> *>(q + row * ld + li * (4 * V)) = w;
    if (li == 0) e[row] = (uint8_t)eb;
}

// Rows too wide for registers (more than 1024 floats): one wave per row, a first read for the maximum, a second one to convert;
// sixteen floats in, 16 bytes out per lane and step.  ld a multiple of 16.
__global__ __launch_bounds__(256) void fp8_rows_wide_kernel(const float *x, uint8_t *q, uint8_t *e, uint64_t rows, uint32_t ld) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t row = (uint64_t)blockIdx.x * 4 + wave;
    if (row >= rows) return;   // (whole waves leave: the butterfly below never misses a lane)
    const float4 *x4 = reinterpret_cast<const float4 *>(x) + row * (ld >> 2);
    const uint32_t pieces = ld >> 4;
    float m = 0.f;
    for (uint32_t p = lane; p < pieces; p += 64)
#pragma unroll
        for (int i = 0; i < 4; ++i) m = amax4(x4[p * 4 + i], m);
    m = group_max<64>(m);
    float inv;
    const uint32_t eb = fp8_row_exponent(m, &inv);
    for (uint32_t p = lane; p < pieces; p += 64) {
        Words<4> w;
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = fp8_pack4(x4[p * 4 + i], inv);
        *reinterpret_cast<Words<4> *>(q + row * ld + p * 16) = w;
    }
    if (lane == 0) e[row] = (uint8_t)eb;
}

template <int GROUP, int V>
static hipError_t launch_fp8_rows_t(const float *x, uint8_t *q, uint8_t *e, uint64_t rows, uint32_t ld, hipStream_t s) {
    constexpr int RPB = 4 * (64 / GROUP);
    hipLaunchKernelGGL((fp8_rows_kernel<GROUP, V>), dim3((uint32_t)((rows + RPB - 1) / RPB)), dim3(256), 0, s, x, q, e, rows, ld);
    return hipGetLastError();
}

// x: rows x ld floats -> q: rows x ld bytes, e: rows bytes.  ld a multiple of 16 (k1_fp8_form asks as much)
hipError_t launch_fp8_rows(const float *x, uint8_t *q, uint8_t *e, uint64_t rows, uint32_t ld, hipStream_t s) {
    if (!rows || !ld) return hipSuccess;
    if ((ld & 15) || (rows + 3) / 4 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (ld <= 32) return launch_fp8_rows_t<8, 1>(x, q, e, rows, ld, s);
    if (ld <= 64) return launch_fp8_rows_t<16, 1>(x, q, e, rows, ld, s);
    if (ld <= 128) return launch_fp8_rows_t<32, 1>(x, q, e, rows, ld, s);
    if (ld <= 256) return launch_fp8_rows_t<64, 1>(x, q, e, rows, ld, s);
    if (ld <= 512) return launch_fp8_rows_t<64, 2>(x, q, e, rows, ld, s);
    if (ld <= 1024) return launch_fp8_rows_t<64, 4>(x, q, e, rows, ld, s);
    hipLaunchKernelGGL(fp8_rows_wide_kernel, dim3((uint32_t)((rows + 3) / 4)), dim3(256), 0, s, x, q, e, rows, ld);
    return hipGetLastError();
}

// ---- the gather ------------------------------------------------------------------------------------------------------------------
// K1's row walk (spmm.hip: spmm_rows8_body) over fp8 rows.  BYTES per lane, edge and chunk: 16 (sixteen features, four float4 sums)
// or 8 (eight features, two).  a.xl / a.xg are not read: the rows come from r.  order / rows, ptr_end, row_clamp, self_mode, both
// accumulate modes and the gridDim.y slabs are K1's.
template <int GROUP, int CHUNKS, int BYTES>
__device__ __forceinline__ void k1_fp8_rows_body(SpmmArgs a, K1Fp8Src r) {
    constexpr int NV = BYTES / 4;        // words per chunk = float4 sums per chunk
    typedef Words<NV> RC;
    constexpr int RPW = 64 / GROUP;      // rows per wave
    constexpr int RPB = 4 * RPW;         // rows per 256-thread block
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int li = lane % GROUP;
    const int gi = lane / GROUP;
    const uint32_t rid = blockIdx.x * RPB + wave * RPW + gi;
    const bool row_ok = rid < (a.rows ? a.rows : a.N);
    uint32_t v = row_ok ? (a.order ? a.order[rid] : rid) : 0;
    if constexpr (GROUP == 64) v = (uint32_t)__builtin_amdgcn_readfirstlane((int)v);

    const uint32_t nchunk = a.ld / BYTES;                    // chunks of BYTES features (NV float4 of out) per row
    const uint32_t c0 = blockIdx.y * (GROUP * CHUNKS) + li;  // first chunk of this lane
    bool act[CHUNKS];
    uint32_t col[CHUNKS];  // inactive lanes gather chunk 0 (valid memory) and never store
    float4 acc[CHUNKS][NV];
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        act[k] = row_ok && (c0 + GROUP * k) < nchunk;
        col[k] = act[k] ? c0 + GROUP * k : 0;
#pragma unroll
        for (int i = 0; i < NV; ++i) acc[k][i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
    if (a.accumulate == 2) {   // second pass of an edge-split aggregation: go on from the first pass's sum
        const float4 *o4 = reinterpret_cast<const float4 *>(a.out);
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k)
            if (act[k])
#pragma unroll
                for (int i = 0; i < NV; ++i) acc[k][i] = o4[((size_t)v * nchunk + col[k]) * NV + i];
    }

    const RC *rows = reinterpret_cast<const RC *>(r.q);

    if (a.self_mode != 0) {
        const float sc = (a.self_mode == 1 && row_ok) ? a.self_scale[v] : 1.f;
        const float se = fp8_scale(r.e[v]);
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k)
            if (act[k]) {
                const RC x = rows[(size_t)v * nchunk + col[k]];
#pragma unroll
                for (int i = 0; i < NV; ++i) {
                    const float4 y = fp8x4_to_float4(x[i], se);
                    acc[k][i] = make_float4(y.x * sc, y.y * sc, y.z * sc, y.w * sc);
                }
            }
    }

    uint64_t e = row_ok ? a.ptr[v] : 0;
    uint64_t end = row_ok ? (a.ptr_end ? a.ptr_end[v] : a.ptr[v + 1]) : 0;
    if (a.row_clamp && end - e > a.row_clamp) end = e + a.row_clamp;   // the rest of a long row: k1_fp8_longrow_kernel
    while (e < end) {
        const int n = (end - e) < (uint64_t)GROUP ? (int)(end - e) : GROUP;
        uint32_t my_idx = 0;
        float my_val = 0.f, my_scale = 0.f;
        if (li < n) {
            my_idx = a.idx[e + li];
            my_val = a.val[e + li];
            my_scale = fp8_scale(r.e[my_idx]);
        }
        int j = 0;
        for (; j + 4 <= n; j += 4) {
            RC x[4][CHUNKS];   // raw E4M3 in flight, widened as they are summed
            float w[4], sc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t s = bcast_u32<GROUP>(my_idx, j + u);
                w[u] = bcast_f32<GROUP>(my_val, j + u);
                sc[u] = bcast_f32<GROUP>(my_scale, j + u);
                const RC *row = rows + (size_t)s * nchunk;
#pragma unroll
                for (int k = 0; k < CHUNKS; ++k) x[u][k] = row[col[k]];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int k = 0; k < CHUNKS; ++k)
#pragma unroll
                    for (int i = 0; i < NV; ++i) acc[k][i] = fma4(w[u], fp8x4_to_float4(x[u][k][i], sc[u]), acc[k][i]);
        }
        for (; j < n; ++j) {
            const uint32_t s = bcast_u32<GROUP>(my_idx, j);
            const float w = bcast_f32<GROUP>(my_val, j);
            const float sc = bcast_f32<GROUP>(my_scale, j);
            const RC *row = rows + (size_t)s * nchunk;
#pragma unroll
            for (int k = 0; k < CHUNKS; ++k) {
                const RC x = row[col[k]];
#pragma unroll
                for (int i = 0; i < NV; ++i) acc[k][i] = fma4(w, fp8x4_to_float4(x[i], sc), acc[k][i]);
            }
        }
        e += n;
    }

    float4 *out4 = reinterpret_cast<float4 *>(a.out);
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k)
        if (act[k]) {
            const size_t o = ((size_t)v * nchunk + col[k]) * NV;
#pragma unroll
            for (int i = 0; i < NV; ++i) {
                if (a.accumulate == 1) {
                    const float4 p = out4[o + i];
                    acc[k][i].x += p.x; acc[k][i].y += p.y; acc[k][i].z += p.z; acc[k][i].w += p.w;
                }
                out4[o + i] = acc[k][i];
            }
        }
}

template <int GROUP, int CHUNKS, int BYTES>
__global__ __launch_bounds__(256) void k1_fp8_rows_kernel(SpmmArgs a, K1Fp8Src r) { k1_fp8_rows_body<GROUP, CHUNKS, BYTES>(a, r); }

template <int GROUP, int CHUNKS, int BYTES>
static hipError_t launch_f8(const SpmmArgs &a, const K1Fp8Src &r, hipStream_t s) {
    constexpr int RPB = 4 * (64 / GROUP);
    const uint32_t nchunk = a.ld / BYTES;
    const uint32_t rows = a.rows ? a.rows : a.N;
    dim3 grid((rows + RPB - 1) / RPB, (nchunk + GROUP * CHUNKS - 1) / (GROUP * CHUNKS));
    if (rows == 0 || nchunk == 0) return hipSuccess;
    hipLaunchKernelGGL((k1_fp8_rows_kernel<GROUP, CHUNKS, BYTES>), grid, dim3(256), 0, s, a, r);
    return hipGetLastError();
}

// slab: option spmm_slab.  Refused where k1_fp8_form has no form or the shadow rows are not 16-byte aligned (the caller asked first).
hipError_t launch_k1_fp8(const SpmmArgs &a, const K1Fp8Src &r, int slab, hipStream_t s) {
    uint32_t lanes = 0, chunks = 0, bytes = 0;
    if (!k1_fp8_form(a.ld, slab > 0 ? (uint32_t)slab : 0u, &lanes, &chunks, &bytes) || (reinterpret_cast<uintptr_t>(r.q) & 15) || !r.e)
        return hipErrorInvalidValue;
    switch (bytes * 1024 + lanes * 4 + chunks) {
    case 8 * 1024 + 8 * 4 + 1: return launch_f8<8, 1, 8>(a, r, s);
    case 8 * 1024 + 16 * 4 + 1: return launch_f8<16, 1, 8>(a, r, s);
    case 16 * 1024 + 8 * 4 + 1: return launch_f8<8, 1, 16>(a, r, s);
    case 16 * 1024 + 16 * 4 + 1: return launch_f8<16, 1, 16>(a, r, s);
    case 16 * 1024 + 32 * 4 + 1: return launch_f8<32, 1, 16>(a, r, s);
    case 16 * 1024 + 64 * 4 + 1: return launch_f8<64, 1, 16>(a, r, s);
    case 16 * 1024 + 64 * 4 + 2: return launch_f8<64, 2, 16>(a, r, s);
    }
    return hipErrorInvalidValue;
}

// ---- long rows (spmm.hip: spmm_longrow_body) -----------------------------------------------------------------------------------
// One workgroup per chunk of LONG_ROW_CHUNK edges: 4 waves x a contiguous quarter of the chunk, whole row width per wave (a lane owns
// one float4 column = one word of four E4M3 per edge; 256 floats of the row per pass), wave partials added in wave order through LDS;
// k1_fp8_longrow_reduce_kernel adds a row's chunk sums to `out` in chunk order.  Per element the additions of the fp32 kernels.
struct LongChunk { uint32_t row; uint32_t pad; uint64_t e0, e1; };   // (6 words per chunk: row_chunks.hpp, plan_long_rows)

__global__ __launch_bounds__(256) void k1_fp8_longrow_kernel(SpmmArgs a, K1Fp8Src r, const LongChunk *chunks, float *partial) {
    extern __shared__ float4 lds4[];                    // [4][nchunk]
    const LongChunk ch = chunks[blockIdx.x];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t nchunk = a.ld >> 2;
    const uint32_t *rows = reinterpret_cast<const uint32_t *>(r.q);
    const uint64_t len = ch.e1 - ch.e0, q = (len + 3) / 4;
    const uint64_t wb = ch.e0 + (uint64_t)wave * q, we = wb + q < ch.e1 ? wb + q : ch.e1;
    for (uint32_t c0 = 0; c0 < nchunk; c0 += 64) {
        const uint32_t col = c0 + lane;
        const bool act = col < nchunk;
        const uint32_t cc = act ? col : 0;
        float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
        uint64_t e = wb;
        for (; e + 4 <= we; e += 4) {
            uint32_t x[4];
            float w[4], sc[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t s = a.idx[e + u];        // wave-uniform
                w[u] = a.val[e + u];
                sc[u] = fp8_scale(r.e[s]);
                x[u] = rows[(size_t)s * nchunk + cc];
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) acc = fma4(w[u], fp8x4_to_float4(x[u], sc[u]), acc);
        }
        for (; e < we; ++e) {
            const uint32_t s = a.idx[e];
            acc = fma4(a.val[e], fp8x4_to_float4(rows[(size_t)s * nchunk + cc], fp8_scale(r.e[s])), acc);
        }
        if (act) lds4[(size_t)wave * nchunk + col] = acc;
    }
    __syncthreads();
    float4 *p4 = reinterpret_cast<float4 *>(partial) + (size_t)blockIdx.x * nchunk;
    for (uint32_t col = threadIdx.x; col < nchunk; col += 256) {
        float4 t = lds4[col];
        for (int w = 1; w < 4; ++w) {
            const float4 u = lds4[(size_t)w * nchunk + col];
            t.x += u.x; t.y += u.y; t.z += u.z; t.w += u.w;
        }
        p4[col] = t;
    }
}

// out[row,:] += sum of the row's chunk partials, in chunk order (one workgroup per long row)
__global__ __launch_bounds__(256) void k1_fp8_longrow_reduce_kernel(float *out, uint32_t ld, const uint32_t *row_ids, const uint32_t *row_chunk_ptr,
                                                                    const float *partial) {
    const uint32_t nchunk = ld >> 2;
    const uint32_t row = row_ids[blockIdx.x], c_beg = row_chunk_ptr[blockIdx.x], c_end = row_chunk_ptr[blockIdx.x + 1];
    const float4 *p4 = reinterpret_cast<const float4 *>(partial);
    float4 *out4 = reinterpret_cast<float4 *>(out) + (size_t)row * nchunk;
    for (uint32_t col = threadIdx.x; col < nchunk; col += 256) {
        float4 acc = out4[col];
        for (uint32_t c = c_beg; c < c_end; ++c) {
            const float4 t = p4[(size_t)c * nchunk + col];
            acc.x += t.x; acc.y += t.y; acc.z += t.z; acc.w += t.w;
        }
        out4[col] = acc;
    }
}

hipError_t launch_k1_fp8_long_rows(const SpmmArgs &a, const K1Fp8Src &r, const LongRowsDev &L, float *partial, hipStream_t s) {
    if (L.nchunks == 0 || a.ld == 0) return hipSuccess;
    if ((a.ld & 3) || !r.q || !r.e) return hipErrorInvalidValue;
    const uint32_t nchunk = a.ld >> 2;
    hipLaunchKernelGGL(k1_fp8_longrow_kernel, dim3(L.nchunks), dim3(256), (size_t)4 * nchunk * sizeof(float4), s, a, r,
                       reinterpret_cast<const LongChunk *>(L.chunks), partial);
    hipLaunchKernelGGL(k1_fp8_longrow_reduce_kernel, dim3(L.nrows), dim3(256), 0, s, a.out, a.ld, L.rows, L.row_chunk_ptr, partial);
    return hipGetLastError();
}

}  // namespace dory
