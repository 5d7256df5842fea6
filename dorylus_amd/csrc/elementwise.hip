// elementwise.hip -- K3/K4/K5/K6/K7: the HBM-bound helpers around the two big
// kernels.  All are streaming kernels (16-B lanes where the layout allows),
// fp32, gfx950.  Reference call sites are cited per kernel; paths are relative
// to the reference's src/graph-server/ unless they start with src/.
#include "ctx.hpp"

namespace dory {

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}

// ---- K3: g = aTg * (1 - tanh(z)^2)  ------------------------------------------
// activateDerivative + Matrix::operator* in vtxNNBackwardGCN
// (commmanager/CPU_comm.cpp:140-143,436-446); cudnnActivationBackward in the
// CUDA backend (GPU-Computation/comp_unit.cu:213-239).
__global__ void tanh_backward_kernel(uint64_t rows, uint32_t cols, const float *aTg, uint32_t lda,
                                     const float *z, uint32_t ldz, float *g, uint32_t ldg) {
    const uint32_t c4 = (cols + 3) / 4;
    const uint64_t n = rows * c4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / c4;
        const uint32_t c = (uint32_t)(i % c4) * 4;
        const float4 a = *reinterpret_cast<const float4 *>(aTg + r * lda + c);
        const float4 zz = *reinterpret_cast<const float4 *>(z + r * ldz + c);
        float4 o;
        float t;
        t = dory_tanh(zz.x); o.x = a.x * (1.f - t * t);
        t = dory_tanh(zz.y); o.y = a.y * (1.f - t * t);
        t = dory_tanh(zz.z); o.z = a.z * (1.f - t * t);
        t = dory_tanh(zz.w); o.w = a.w * (1.f - t * t);
        // padding columns of aTg are zero, so padding of g stays zero
        *reinterpret_cast<float4 *>(g + r * ldg + c) = o;
    }
}

hipError_t launch_tanh_backward(uint64_t rows, uint32_t cols, const float *aTg, uint32_t lda,
                                const float *z, uint32_t ldz, float *g, uint32_t ldg, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    if ((lda | ldz | ldg) & 3u) return hipErrorInvalidValue;   // 16-byte lanes: a one-column tensor (ld = 1) would be read and written past its rows
    const uint64_t n = rows * ((cols + 3) / 4);
    int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    hipLaunchKernelGGL(tanh_backward_kernel, dim3(blocks), dim3(256), 0, s, rows, cols, aTg, lda, z, ldz, g, ldg);
    return hipGetLastError();
}

// h = tanh(z) on its own: the transform-first order computes z with the SpMM, not the GEMM whose
// epilogue normally applies the activation (same tanhf as that epilogue)
__global__ void tanh_forward_kernel(uint64_t rows, uint32_t cols, const float *z, uint32_t ldz, float *h, uint32_t ldh) {
    const uint64_t n = rows * cols;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / cols;
        const uint32_t c = (uint32_t)(i % cols);
        h[r * ldh + c] = dory_tanh(z[r * ldz + c]);
    }
}
hipError_t launch_tanh_forward(uint64_t rows, uint32_t cols, const float *z, uint32_t ldz, float *h, uint32_t ldh,
                               hipStream_t s) {
    if (rows == 0 || cols == 0) return hipSuccess;
    const uint64_t n = rows * cols;
    int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    hipLaunchKernelGGL(tanh_forward_kernel, dim3(blocks), dim3(256), 0, s, rows, cols, z, ldz, h, ldh);
    return hipGetLastError();
}

// ---- K4: softmax + maskout quirk + (p - lab) / denom  ---------------------------
// softmax (CPU_comm.cpp:276-297: max-subtracted, denominator seeded with 1e-20),
// maskout (CPU_comm.cpp:464-471: copies (rows - stt) FLOATS of the dense label
// tensor over the dense prediction tensor starting at row stt -- reproduced as a
// flat dense-index range), hadamardSub + "/= globalVtxCnt * TRAIN_PORTION"
// (CPU_comm.cpp:121-122).  CUDA backend: cudnnSoftmaxForward + thrust minus +
// cublasSscal + cudaMemcpy maskout (comp_unit.cu:161-210,331-346).
// LPR lanes per row (64, 32, 16 or 8: the smallest that holds a row of up to 64 / 32 / 16 / 8 classes, so a wave
// covers 1-8 rows and no lane idles on narrow label sets); lane c owns columns c, c+LPR, ...  The xor-shuffle trees
// descend from LPR/2, i.e. the sums are the ones the 64-lane tree gives with the unused lanes at zero.
template <int LPR>
__global__ __launch_bounds__(256) void softmax_xent_kernel(
    uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab, uint32_t ldl,
    float *d, uint32_t ldd, float inv_mode_denom, uint64_t mask_first, uint64_t mask_count,
    int sub_only) {
    const int lane = threadIdx.x % LPR;
    const uint32_t row = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (row >= rows) return;
    const float *zr = z + (size_t)row * ldz;
    float mx = -INFINITY;
    for (uint32_t c = lane; c < cols; c += LPR) mx = fmaxf(mx, zr[c]);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (uint32_t c = lane; c < cols; c += LPR) sum += expf(zr[c] - mx);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    sum += 1e-20f;
    const float *lr = lab + (size_t)row * ldl;
    float *dr = d + (size_t)row * ldd;
    for (uint32_t c = lane; c < cols; c += LPR) {
        float p = expf(zr[c] - mx) / sum;
        const float l = lr[c];
        if (sub_only) {  // predictGAT (engine/ops/gat_ops.cpp:246-265): softmax - label
            dr[c] = p - l;
        } else {
            const uint64_t flat = (uint64_t)row * cols + c;
            if (flat >= mask_first && flat - mask_first < mask_count) p = l;
            dr[c] = (p - l) / inv_mode_denom;
        }
    }
}

template <int LPR, bool BF16>
__global__ __launch_bounds__(256) void softmax_rows_send_kernel(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab,
                                                                uint32_t ldl, float *d, uint32_t ldd, float inv_mode_denom, uint64_t mask_first,
                                                                uint64_t mask_count, int sub_only, GemmSend sd);

static void launch_softmax_rows(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab,
                                uint32_t ldl, float *d, uint32_t ldd, float denom, uint64_t mask_first,
                                uint64_t mask_count, int sub_only, hipStream_t s, const GemmSend *sd = nullptr) {
    if (sd) {   // dory_halo_fused_pack_rowwise: the send forms, at the lanes per row of the plain ones
#define SOFTMAX_SEND(L)                                                                                                                  \
    do {                                                                                                                                 \
        if (sd->bf16) hipLaunchKernelGGL((softmax_rows_send_kernel<L, true>), dim3((rows + 256 / L - 1) / (256 / L)), dim3(256), 0, s, rows, cols, \
                                         z, ldz, lab, ldl, d, ldd, denom, mask_first, mask_count, sub_only, *sd);                        \
        else hipLaunchKernelGGL((softmax_rows_send_kernel<L, false>), dim3((rows + 256 / L - 1) / (256 / L)), dim3(256), 0, s, rows, cols, z,     \
                                ldz, lab, ldl, d, ldd, denom, mask_first, mask_count, sub_only, *sd);                                    \
    } while (0)
        if (cols <= 8) SOFTMAX_SEND(8);
        else if (cols <= 16) SOFTMAX_SEND(16);
        else if (cols <= 32) SOFTMAX_SEND(32);
        else if (cols <= 48) SOFTMAX_SEND(16);
        else SOFTMAX_SEND(64);
#undef SOFTMAX_SEND
        return;
    }
#define SOFTMAX_LPR(L)                                                                                              \
    hipLaunchKernelGGL(softmax_xent_kernel<L>, dim3((rows + 256 / L - 1) / (256 / L)), dim3(256), 0, s, rows, cols, z, \
                       ldz, lab, ldl, d, ldd, denom, mask_first, mask_count, sub_only)
    if (cols <= 8) SOFTMAX_LPR(8);
    else if (cols <= 16) SOFTMAX_LPR(16);
    else if (cols <= 32) SOFTMAX_LPR(32);
    else if (cols <= 48) SOFTMAX_LPR(16);   // e.g. Reddit's 41 classes: three columns per lane, four rows per wave (81 -> 49 us at
                                            // 232 965 rows against one row per wave with 23 idle lanes and six-step trees)
    else SOFTMAX_LPR(64);
#undef SOFTMAX_LPR
}

// CPUComm::getTrainStat (CPU_comm.cpp:448-462): over validation rows
// [val_stt, val_end): acc += lab[argmax(pred)], loss -= log(pred[argmax(lab)]).
// One row per thread with the reference's own sequential arithmetic, but the rows of a block are staged through
// LDS with coalesced loads first (a thread reading its row straight from HBM touches 64 lines per instruction);
// per-block tree sums, then one block adds the block partials in a fixed order -> deterministic.  (thrust functors
// in the CUDA backend: comp_unit.cu:258-312, cuda_ops.cuh:45-113.)
constexpr int STAT_ROWS_MAX = 64;   // rows per block (fewer when the label set is so wide that 64 rows do not fit LDS)
static uint32_t stat_rows_per_block(uint32_t cols) {
    uint32_t rb = STAT_ROWS_MAX;
    while (rb > 1 && (size_t)2 * rb * (cols + 1) * sizeof(float) > 48 * 1024) rb >>= 1;
    return rb;
}
__global__ __launch_bounds__(256) void train_stat_kernel(uint32_t cols, const float *z, uint32_t ldz,
                                                         const float *lab, uint32_t ldl,
                                                         uint32_t val_stt, uint32_t val_end,
                                                         float *partial, uint32_t STAT_ROWS) {
    extern __shared__ float sm[];            // [STAT_ROWS][cols+1] z, then the same for lab
    const uint32_t pitch = cols + 1;
    float *sz = sm, *sl = sm + STAT_ROWS * pitch;
    const uint32_t r0 = val_stt + blockIdx.x * STAT_ROWS;
    for (uint32_t i = threadIdx.x; i < STAT_ROWS * cols; i += 256) {
        const uint32_t rr = i / cols, c = i % cols;
        const uint32_t r = r0 + rr;
        sz[rr * pitch + c] = r < val_end ? z[(size_t)r * ldz + c] : 0.f;
        sl[rr * pitch + c] = r < val_end ? lab[(size_t)r * ldl + c] : 0.f;
    }
    __syncthreads();
    __shared__ float sa[STAT_ROWS_MAX], sls[STAT_ROWS_MAX];
    if (threadIdx.x < STAT_ROWS) {
        float acc = 0.f, loss = 0.f;
        if (r0 + threadIdx.x < val_end) {
            const float *zr = sz + threadIdx.x * pitch;
            const float *lr = sl + threadIdx.x * pitch;
            float mx = zr[0];
            uint32_t am = 0, al = 0;
            float lmax = lr[0];
            for (uint32_t c = 1; c < cols; ++c) {
                if (zr[c] > mx) { mx = zr[c]; am = c; }      // argmax(pred) == argmax(z), first max
                if (lr[c] > lmax) { lmax = lr[c]; al = c; }
            }
            float den = 1e-20f;
            for (uint32_t c = 0; c < cols; ++c) den += expf(zr[c] - mx);
            acc = lr[am];
            loss = -logf(expf(zr[al] - mx) / den);
        }
        sa[threadIdx.x] = acc;
        sls[threadIdx.x] = loss;
    }
    __syncthreads();
    for (int o = (int)STAT_ROWS / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sls[threadIdx.x] += sls[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        partial[2 * blockIdx.x] = sa[0];
        partial[2 * blockIdx.x + 1] = sls[0];
    }
}
// one block: thread t adds partials t, t+256, ... in order, then a fixed tree over the 256 threads
__global__ __launch_bounds__(256) void train_stat_final_kernel(const float *partial, uint32_t nb, float *stat) {
    __shared__ float sa[256], sl[256];
    float a = 0.f, l = 0.f;
    for (uint32_t b = threadIdx.x; b < nb; b += 256) {
        a += partial[2 * b];
        l += partial[2 * b + 1];
    }
    sa[threadIdx.x] = a;
    sl[threadIdx.x] = l;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            sa[threadIdx.x] += sa[threadIdx.x + o];
            sl[threadIdx.x] += sl[threadIdx.x + o];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        stat[0] = sa[0];
        stat[1] = sl[0];
    }
}

size_t softmax_xent_scratch_bytes(uint32_t cols, uint32_t val_rows) {   // per-block partials of the validation statistics
    const uint32_t rb = stat_rows_per_block(cols);
    return (size_t)(2 * ((val_rows + rb - 1) / rb) + 64) * sizeof(float);
}

// the validation statistics of launch_softmax_xent and of its send form
static void launch_train_stat(uint32_t cols, const float *z, uint32_t ldz, const float *lab, uint32_t ldl, uint32_t val_stt, uint32_t val_end,
                              float *stat, float *stat_partial, hipStream_t s) {
    const uint32_t rb = stat_rows_per_block(cols);
    const uint32_t nb = (val_end - val_stt + rb - 1) / rb;
    if (nb)
        hipLaunchKernelGGL(train_stat_kernel, dim3(nb), dim3(256), (size_t)2 * rb * (cols + 1) * sizeof(float), s, cols, z,
                           ldz, lab, ldl, val_stt, val_end, stat_partial, rb);
    hipLaunchKernelGGL(train_stat_final_kernel, dim3(1), dim3(256), 0, s, stat_partial, nb, stat);
}

hipError_t launch_softmax_xent(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz,
                               const float *lab, uint32_t ldl, float *d, uint32_t ldd, float denom,
                               uint32_t val_stt, uint32_t val_end, uint64_t mask_first,
                               uint64_t mask_count, float *stat, float *stat_partial, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    launch_train_stat(cols, z, ldz, lab, ldl, val_stt, val_end, stat, stat_partial, s);
    launch_softmax_rows(rows, cols, z, ldz, lab, ldl, d, ldd, denom, mask_first, mask_count, 0, s);
    return hipGetLastError();
}

hipError_t launch_softmax_sub(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz,
                              const float *lab, uint32_t ldl, float *out, uint32_t ldo, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    launch_softmax_rows(rows, cols, z, ldz, lab, ldl, out, ldo, 1.f, 0, 0, 1, s);
    return hipGetLastError();
}

// ---- K3 / K4, send forms (dory_halo_fused_pack_rowwise) --------------------------------------------------------------------------
// The row-wise producers of a tensor that is the source of the next exchange: each computes and stores its tensor exactly as its
// parent above does (the same expressions on the same operands), and stores row r once more into every slot
// row_slots[row_ptr[r] .. row_ptr[r + 1]) of the packed send buffer, in the wire format of the moment (GemmSend, ctx.hpp) -- what
// the pack kernel would copy out of the tensor afterwards:
//   SEND_F4   fp32, w a multiple of 4 (the padded row, w == ld, or an exact row whose cols is one): 16-byte stores
//   SEND_F1   fp32 exact rows with cols % 4 != 0 (w == cols): a slot's row starts on a 4-byte boundary only -- dword stores
//   SEND_BF16 w 2-byte elements (a multiple of 4): pack_bf16x2 of the values, zeros in [cols, w) -- 8-byte stores (tanh forms),
//             4-byte stores of a lane pair's dword (softmax forms)
// Columns [cols, w) of a padded fp32 row get what the tensor holds there: the zeros of its padding (tanh_backward: what it has just
// stored into the last quad).  Most rows go to no peer: the slot range is loaded once per lane and quad (softmax: per lane and
// row), outside every loop over elements, and an empty one skips the rest.  Offsets into the send buffer are 64-bit.
enum { SEND_F4 = 0, SEND_F1 = 1, SEND_BF16 = 2 };
// the quad of columns c .. c + 3 (c a multiple of 4, c < w) of a row into the slots [s0, s1); v: the wire's values (zeros where it has them)
template <int FORM>
__device__ __forceinline__ void send_quad(const GemmSend &sd, uint32_t s0, uint32_t s1, uint32_t c, float4 v) {
    if (FORM == SEND_BF16) {
        const uint2 bits = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
        uint16_t *buf = reinterpret_cast<uint16_t *>(sd.buf);
        for (uint32_t s = s0; s < s1; ++s) *reinterpret_cast<uint2 *>(buf + (size_t)sd.row_slots[s] * sd.w + c) = bits;
    } else if (FORM == SEND_F4) {
        for (uint32_t s = s0; s < s1; ++s) *reinterpret_cast<float4 *>(sd.buf + (size_t)sd.row_slots[s] * sd.w + c) = v;
    } else {
        const float e[4] = {v.x, v.y, v.z, v.w};
        for (uint32_t s = s0; s < s1; ++s) {
            float *p = sd.buf + (size_t)sd.row_slots[s] * sd.w + c;
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (c + k < sd.w) p[k] = e[k];
        }
    }
}
// quads per row of a send form: those of the tensor (the parent's) or of the wire's row, whichever are more (a padded row: ld / 4)
__host__ __device__ __forceinline__ uint32_t send_quads(uint32_t cols, uint32_t w) { return ((cols > w ? cols : w) + 3u) / 4u; }

// g = aTg * (1 - tanh(z)^2) as tanh_backward_kernel, a float4 per lane
template <int FORM>
__global__ __launch_bounds__(256) void tanh_backward_send_kernel(uint64_t rows, uint32_t cols, const float *aTg, uint32_t lda, const float *z,
                                                                 uint32_t ldz, float *g, uint32_t ldg, GemmSend sd) {
    const uint32_t c4 = (cols + 3) / 4, q4 = send_quads(cols, sd.w);
    const uint64_t n = rows * q4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / q4;
        const uint32_t c = (uint32_t)(i % q4) * 4;
        const uint32_t s0 = sd.row_ptr[r], s1 = sd.row_ptr[r + 1];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < c4 * 4) {
            const float4 a = *reinterpret_cast<const float4 *>(aTg + r * lda + c);
            const float4 zz = *reinterpret_cast<const float4 *>(z + r * ldz + c);
            float t;
            t = dory_tanh(zz.x); o.x = a.x * (1.f - t * t);
            t = dory_tanh(zz.y); o.y = a.y * (1.f - t * t);
            t = dory_tanh(zz.z); o.z = a.z * (1.f - t * t);
            t = dory_tanh(zz.w); o.w = a.w * (1.f - t * t);
            *reinterpret_cast<float4 *>(g + r * ldg + c) = o;
        }
        if (s0 == s1 || c >= sd.w) continue;
        if (FORM == SEND_BF16) {   // (the pack reads `cols` columns: zeros behind them)
            if (c + 1 >= cols) o.y = 0.f;
            if (c + 2 >= cols) o.z = 0.f;
            if (c + 3 >= cols) o.w = 0.f;
            if (c >= cols) o.x = 0.f;
        }
        send_quad<FORM>(sd, s0, s1, c, o);
    }
}

// h = tanh(z) as tanh_forward_kernel, but a float4 per lane (ldz, ldh multiples of 4): columns >= cols of h are not written
template <int FORM>
__global__ __launch_bounds__(256) void tanh_forward_send_kernel(uint64_t rows, uint32_t cols, const float *z, uint32_t ldz, float *h, uint32_t ldh,
                                                                GemmSend sd) {
    const uint32_t q4 = send_quads(cols, sd.w);
    const uint64_t n = rows * q4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / q4;
        const uint32_t c = (uint32_t)(i % q4) * 4;
        const uint32_t s0 = sd.row_ptr[r], s1 = sd.row_ptr[r + 1];
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if (c < cols) {
            const float4 zz = *reinterpret_cast<const float4 *>(z + r * ldz + c);   // (c + 3 < ldz: ldz >= cols, a multiple of 4)
            float *hr = h + r * ldh + c;
            o.x = dory_tanh(zz.x);
            if (c + 3 < cols) {
                o.y = dory_tanh(zz.y); o.z = dory_tanh(zz.z); o.w = dory_tanh(zz.w);
                *reinterpret_cast<float4 *>(hr) = o;
            } else {
                hr[0] = o.x;
                if (c + 1 < cols) hr[1] = o.y = dory_tanh(zz.y);
                if (c + 2 < cols) hr[2] = o.z = dory_tanh(zz.z);
            }
        }
        if (s0 == s1 || c >= sd.w) continue;
        send_quad<FORM>(sd, s0, s1, c, o);
    }
}

// softmax_xent_kernel<LPR> with the row's slots: lane c owns columns c, c + LPR, ... as there; the loop that stores the row runs to
// the wire's width on every lane of the row's group, so that in the bf16 form an even lane can take its right neighbour's value by
// DPP (lane_right: LPR is even, so column parity is lane parity and both lanes of a pair take every turn together) and store the
// pair's dword
template <int LPR, bool BF16>
__global__ __launch_bounds__(256) void softmax_rows_send_kernel(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab,
                                                                uint32_t ldl, float *d, uint32_t ldd, float inv_mode_denom, uint64_t mask_first,
                                                                uint64_t mask_count, int sub_only, GemmSend sd) {
    const int lane = threadIdx.x % LPR;
    const uint32_t row = blockIdx.x * (256 / LPR) + threadIdx.x / LPR;
    if (row >= rows) return;
    const uint32_t s0 = sd.row_ptr[row], s1 = sd.row_ptr[row + 1];
    const uint32_t slot0 = s0 != s1 ? sd.row_slots[s0] : 0u;   // (the first slot -- for most rows that travel the only one -- ahead of the arithmetic)
    const float *zr = z + (size_t)row * ldz;
    float mx = -INFINITY;
    for (uint32_t c = lane; c < cols; c += LPR) mx = fmaxf(mx, zr[c]);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o, 64));
    float sum = 0.f;
    for (uint32_t c = lane; c < cols; c += LPR) sum += expf(zr[c] - mx);
#pragma unroll
    for (int o = LPR / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    sum += 1e-20f;
    const float *lr = lab + (size_t)row * ldl;
    float *dr = d + (size_t)row * ldd;
    const uint32_t cend = s0 != s1 && sd.w > cols ? sd.w : cols;   // (the same on every lane of the row)
    for (uint32_t c0 = 0; c0 < cend; c0 += LPR) {
        const uint32_t c = c0 + lane;
        float v = 0.f;
        if (c < cols) {
            float p = expf(zr[c] - mx) / sum;
            const float l = lr[c];
            if (sub_only) {
                v = p - l;
            } else {
                const uint64_t flat = (uint64_t)row * cols + c;
                if (flat >= mask_first && flat - mask_first < mask_count) p = l;
                v = (p - l) / inv_mode_denom;
            }
            dr[c] = v;
        }
        if (BF16) {
            const uint32_t bits = pack_bf16x2(v, lane_right(v));
            if (!(lane & 1) && c < sd.w) {
                uint16_t *buf = reinterpret_cast<uint16_t *>(sd.buf);
                if (s0 != s1) *reinterpret_cast<uint32_t *>(buf + (size_t)slot0 * sd.w + c) = bits;
                for (uint32_t s = s0 + 1; s < s1; ++s) *reinterpret_cast<uint32_t *>(buf + (size_t)sd.row_slots[s] * sd.w + c) = bits;
            }
        } else if (c < sd.w) {
            if (s0 != s1) sd.buf[(size_t)slot0 * sd.w + c] = v;
            for (uint32_t s = s0 + 1; s < s1; ++s) sd.buf[(size_t)sd.row_slots[s] * sd.w + c] = v;
        }
    }
}

// the wire format a GemmSend asks of the tanh forms
static int send_form(const GemmSend &sd) { return sd.bf16 ? SEND_BF16 : (sd.w & 3u) ? SEND_F1 : SEND_F4; }

hipError_t launch_tanh_backward_send(uint64_t rows, uint32_t cols, const float *aTg, uint32_t lda, const float *z, uint32_t ldz, float *g,
                                     uint32_t ldg, const GemmSend &sd, hipStream_t s, bool *fused) {
    *fused = false;
    if (rows == 0 || cols == 0 || ((lda | ldz | ldg) & 3u) || (sd.bf16 && (sd.w & 3u)))
        return launch_tanh_backward(rows, cols, aTg, lda, z, ldz, g, ldg, s);
    const uint64_t n = rows * send_quads(cols, sd.w);
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    switch (send_form(sd)) {
    case SEND_F4: hipLaunchKernelGGL(tanh_backward_send_kernel<SEND_F4>, dim3(blocks), dim3(256), 0, s, rows, cols, aTg, lda, z, ldz, g, ldg, sd); break;
    case SEND_F1: hipLaunchKernelGGL(tanh_backward_send_kernel<SEND_F1>, dim3(blocks), dim3(256), 0, s, rows, cols, aTg, lda, z, ldz, g, ldg, sd); break;
    default: hipLaunchKernelGGL(tanh_backward_send_kernel<SEND_BF16>, dim3(blocks), dim3(256), 0, s, rows, cols, aTg, lda, z, ldz, g, ldg, sd); break;
    }
    *fused = true;
    return hipGetLastError();
}
hipError_t launch_tanh_forward_send(uint64_t rows, uint32_t cols, const float *z, uint32_t ldz, float *h, uint32_t ldh, const GemmSend &sd,
                                    hipStream_t s, bool *fused) {
    *fused = false;
    if (rows == 0 || cols == 0 || ((ldz | ldh) & 3u) || (sd.bf16 && (sd.w & 3u))) return launch_tanh_forward(rows, cols, z, ldz, h, ldh, s);
    const uint64_t n = rows * send_quads(cols, sd.w);
    const int blocks = (int)((n + 255) / 256 < 8192 ? (n + 255) / 256 : 8192);
    switch (send_form(sd)) {
    case SEND_F4: hipLaunchKernelGGL(tanh_forward_send_kernel<SEND_F4>, dim3(blocks), dim3(256), 0, s, rows, cols, z, ldz, h, ldh, sd); break;
    case SEND_F1: hipLaunchKernelGGL(tanh_forward_send_kernel<SEND_F1>, dim3(blocks), dim3(256), 0, s, rows, cols, z, ldz, h, ldh, sd); break;
    default: hipLaunchKernelGGL(tanh_forward_send_kernel<SEND_BF16>, dim3(blocks), dim3(256), 0, s, rows, cols, z, ldz, h, ldh, sd); break;
    }
    *fused = true;
    return hipGetLastError();
}
hipError_t launch_softmax_xent_send(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab, uint32_t ldl, float *d,
                                    uint32_t ldd, float denom, uint32_t val_stt, uint32_t val_end, uint64_t mask_first, uint64_t mask_count,
                                    float *stat, float *stat_partial, const GemmSend &sd, hipStream_t s, bool *fused) {
    *fused = false;
    if (rows == 0 || cols == 0 || (sd.bf16 && (sd.w & 3u)))
        return launch_softmax_xent(rows, cols, z, ldz, lab, ldl, d, ldd, denom, val_stt, val_end, mask_first, mask_count, stat, stat_partial, s);
    launch_train_stat(cols, z, ldz, lab, ldl, val_stt, val_end, stat, stat_partial, s);
    launch_softmax_rows(rows, cols, z, ldz, lab, ldl, d, ldd, denom, mask_first, mask_count, 0, s, &sd);
    *fused = true;
    return hipGetLastError();
}
hipError_t launch_softmax_sub_send(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab, uint32_t ldl, float *out,
                                   uint32_t ldo, const GemmSend &sd, hipStream_t s, bool *fused) {
    *fused = false;
    if (rows == 0 || cols == 0 || (sd.bf16 && (sd.w & 3u))) return launch_softmax_sub(rows, cols, z, ldz, lab, ldl, out, ldo, s);
    launch_softmax_rows(rows, cols, z, ldz, lab, ldl, out, ldo, 1.f, 0, 0, 1, s, &sd);
    *fused = true;
    return hipGetLastError();
}

// ---- synthetic inputs -----------------------------------------------------------
// counter RNG: splitmix64(seed ^ (global_row * cols + col)) -> U[lo, hi); the same
// value for a vertex whichever partition holds it (row ids are global ids).
__device__ __forceinline__ uint64_t splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return x ^ (x >> 31);
}

__global__ void fill_uniform_kernel(float *d, uint64_t rows, uint32_t cols, uint32_t ld,
                                    const uint32_t *row_ids, uint64_t seed, float lo, float hi) {
    const uint64_t n = rows * ld;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / ld;
        const uint32_t c = (uint32_t)(i % ld);
        float v = 0.f;
        if (c < cols) {
            const uint64_t gr = row_ids ? row_ids[r] : r;
            const uint64_t h = splitmix64(seed ^ (gr * cols + c));
            const float u = (float)(h >> 40) * (1.0f / 16777216.0f);  // 24 bits -> [0,1)
            v = lo + (hi - lo) * u;
        }
        d[i] = v;
    }
}

hipError_t launch_fill_uniform(float *d, uint64_t rows, uint32_t cols, uint32_t ld, uint64_t seed,
                               float lo, float hi, hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(fill_uniform_kernel, dim3(2048), dim3(256), 0, s, d, rows, cols, ld,
                       (const uint32_t *)nullptr, seed, lo, hi);
    return hipGetLastError();
}

hipError_t launch_fill_uniform_ids(float *d, uint64_t rows, uint32_t cols, uint32_t ld,
                                   const uint32_t *row_ids, uint64_t seed, float lo, float hi,
                                   hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(fill_uniform_kernel, dim3(2048), dim3(256), 0, s, d, rows, cols, ld, row_ids,
                       seed, lo, hi);
    return hipGetLastError();
}

// one-hot expansion of u32 labels (Engine::readLabelsFile, engine/utils.cpp:559-596)
__global__ void onehot_kernel(float *d, uint64_t rows, uint32_t cols, uint32_t ld, const uint32_t *labels) {
    const uint64_t n = rows * ld;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / ld;
        const uint32_t c = (uint32_t)(i % ld);
        d[i] = (c < cols && labels[r] == c) ? 1.f : 0.f;
    }
}

hipError_t launch_onehot(float *d, uint64_t rows, uint32_t cols, uint32_t ld, const uint32_t *labels,
                         hipStream_t s) {
    if (rows == 0) return hipSuccess;
    hipLaunchKernelGGL(onehot_kernel, dim3(1024), dim3(256), 0, s, d, rows, cols, ld, labels);
    return hipGetLastError();
}

// dense (lds == cols) <-> padded (ldd) row copies; destination padding is zeroed
__global__ void pad_copy_kernel(float *dst, uint32_t ldd, const float *src, uint32_t lds, uint64_t rows,
                                uint32_t cols) {
    const uint64_t n = rows * ldd;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t r = i / ldd;
        const uint32_t c = (uint32_t)(i % ldd);
        dst[i] = c < cols ? src[r * lds + c] : 0.f;
    }
}

// out[v,:] = base[v,:] + rs[v] * S[v,:]   (base = out itself when accumulating, x otherwise): what is left of a GAT-prototype
// aggregation once the unweighted neighbour sum S is known (abi_stages.hip: the reference's edge scores depend on the destination only)
__global__ __launch_bounds__(256) void row_axpy_kernel(float *out, const float *S, const float *rs, const float *x, uint32_t ld4, uint64_t n4) {
    float4 *o4 = reinterpret_cast<float4 *>(out);
    const float4 *s4 = reinterpret_cast<const float4 *>(S), *x4 = reinterpret_cast<const float4 *>(x ? x : out);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x) {
        const float r = rs[i / ld4];
        const float4 b = x4[i], sv = s4[i];
        o4[i] = make_float4(fmaf(r, sv.x, b.x), fmaf(r, sv.y, b.y), fmaf(r, sv.z, b.z), fmaf(r, sv.w, b.w));
    }
}
hipError_t launch_row_axpy(float *out, const float *S, const float *rs, const float *x /* nullptr: out += */, uint64_t rows, uint32_t ld,
                           hipStream_t s) {
    if (rows == 0 || ld == 0) return hipSuccess;
    if (ld & 3) return hipErrorInvalidValue;
    const uint64_t n4 = rows * (ld >> 2);
    hipLaunchKernelGGL(row_axpy_kernel, dim3((uint32_t)std::min<uint64_t>(8192, (n4 + 255) / 256)), dim3(256), 0, s, out, S, rs, x, ld >> 2, n4);
    return hipGetLastError();
}

// out[v,:] = xb[v,:] + rs[v] * S[v,:] with the self row xb read from bf16 rows (dory_gat_bf16_gather: the shadow rows the
// neighbour sum S was gathered from, 8 bytes per four features): row_axpy_kernel's fmaf per element on the expanded values
__global__ __launch_bounds__(256) void row_axpy_bf16_kernel(float *out, const float *S, const float *rs, const uint2 *xb, uint32_t ld4, uint64_t n4) {
    float4 *o4 = reinterpret_cast<float4 *>(out);
    const float4 *s4 = reinterpret_cast<const float4 *>(S);
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x) {
        const float r = rs[i / ld4];
        const uint2 xr = xb[i];
        const float4 sv = s4[i];
        const float4 b = make_float4(__uint_as_float(xr.x << 16), __uint_as_float(xr.x & 0xFFFF0000u), __uint_as_float(xr.y << 16),
                                     __uint_as_float(xr.y & 0xFFFF0000u));
        o4[i] = make_float4(fmaf(r, sv.x, b.x), fmaf(r, sv.y, b.y), fmaf(r, sv.z, b.z), fmaf(r, sv.w, b.w));
    }
}
hipError_t launch_row_axpy_bf16(float *out, const float *S, const float *rs, const uint16_t *xb, uint64_t rows, uint32_t ld, hipStream_t s) {
    if (rows == 0 || ld == 0) return hipSuccess;
    if ((ld & 3) || !xb) return hipErrorInvalidValue;
    const uint64_t n4 = rows * (ld >> 2);
    hipLaunchKernelGGL(row_axpy_bf16_kernel, dim3((uint32_t)std::min<uint64_t>(8192, (n4 + 255) / 256)), dim3(256), 0, s, out, S, rs,
                       reinterpret_cast<const uint2 *>(xb), ld >> 2, n4);
    return hipGetLastError();
}

// option gcn_bf16_gather: the rows an aggregation reads, rounded to bf16 (nearest even; v_cvt_pk_bf16_f32), into the
// context's shadow buffer -- every element of an ld-wide row, so that padding columns stay 0 (pack_bf16x2: ctx.hpp)
__global__ __launch_bounds__(256) void bf16_rows_kernel(const float4 *x, uint2 *y, uint64_t n4) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += (uint64_t)gridDim.x * blockDim.x) {
        const float4 v = x[i];
        y[i] = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
    }
}
hipError_t launch_bf16_rows(const float *x, uint16_t *y, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (n & 3) return hipErrorInvalidValue;
    const uint64_t n4 = n >> 2;
    hipLaunchKernelGGL(bf16_rows_kernel, dim3((uint32_t)std::min<uint64_t>(8192, (n4 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<const float4 *>(x), reinterpret_cast<uint2 *>(y), n4);
    return hipGetLastError();
}

hipError_t launch_pad_copy(float *dst, uint32_t ldd, const float *src, uint32_t lds, uint64_t rows,
                           uint32_t cols, hipStream_t s) {
    if (rows == 0 || ldd == 0) return hipSuccess;
    hipLaunchKernelGGL(pad_copy_kernel, dim3(2048), dim3(256), 0, s, dst, ldd, src, lds, rows, cols);
    return hipGetLastError();
}

// ---- K5: GAT edge kernels -----------------------------------------------------------
// edgNNForwardGAT (CPU_comm.cpp:190-203) = expandDot (299-319) + leakyRelu (384-395):
//   az[e] = z[dst(e),:] . a ;  A[e] = az > 0 ? az : 0.01 az,  dst(e) = owning column.
// All edges of a column share the value, so one wave computes the row dot once
// and streams it over the column's edge range (no csrRowInd gather as in
// GPU-Computation/comp_server.cu:255-262, comp_unit.cu:93-134).
__global__ __launch_bounds__(256) void edge_forward_gat_kernel(uint32_t N, uint32_t F,
                                                               const uint64_t *colptr, const float *z,
                                                               uint32_t ldz, const float *a, float *az,
                                                               float *A, float *arow, float *azrow) {
    const int lane = threadIdx.x & 63;
    const uint32_t v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;
    const float *zr = z + (size_t)v * ldz;
    float s = 0.f;
    for (uint32_t j = lane; j < F; j += 64) s = fmaf(zr[j], a[j], s);
    s = wave_sum(s);
    const float act = s > 0.f ? s : 0.01f * s;
    if (az)      // (nullptr: the per-edge copies are written on demand, expand_rows_to_edges)
        for (uint64_t e = colptr[v] + lane; e < colptr[v + 1]; e += 64) {
            az[e] = s;
            A[e] = act;
        }
    if (lane == 0) {
        arow[v] = act;   // every edge of column v carries the same weight
        if (azrow) azrow[v] = s;
    }
}

// per-edge copy of a per-destination value: out[e] = row[dst(e)] for every in-edge of every local vertex
__global__ __launch_bounds__(256) void expand_rows_to_edges_kernel(uint32_t N, const uint64_t *colptr, const float *row, float *out) {
    const int lane = threadIdx.x & 63;
    const uint32_t v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;
    const float x = row[v];
    for (uint64_t e = colptr[v] + lane; e < colptr[v + 1]; e += 64) out[e] = x;
}
hipError_t launch_expand_rows_to_edges(uint32_t N, const uint64_t *colptr, const float *row, float *out, hipStream_t s) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(expand_rows_to_edges_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, colptr, row, out);
    return hipGetLastError();
}

hipError_t launch_edge_forward_gat(uint32_t N, uint32_t F, const uint64_t *colptr, const float *z,
                                   uint32_t ldz, const float *a, float *az, float *A, float *arow,
                                   hipStream_t s, float *azrow) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(edge_forward_gat_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, F, colptr, z, ldz, a, az, A, arow, azrow);
    return hipGetLastError();
}

// edgNNBackwardGAT (CPU_comm.cpp:205-242):
//   dLRelu[e] = az[e] > 0 ? 1 : .01 ;  dAct[e,:] = grad[dst(e),:] * dLRelu[e]
//   dA[e] = dAct[e,:] . a ;  r[j] = sum_e dAct[e,j]     (the E x F dAct is never built)
// Per column v: s_v = dLRelu of its edges, t_v = s_v * (grad[v,:] . a);
// dA[e] = t_v; cw[v] = deg(v) * s_v is the column weight for r = grad^T cw.
__global__ __launch_bounds__(256) void edge_backward_gat_kernel(uint32_t N, uint32_t F,
                                                                const uint64_t *colptr,
                                                                const float *grad, uint32_t ldg,
                                                                const float *az, const float *a,
                                                                float *dA, float *cw, float *drow, const float *azrow) {
    const int lane = threadIdx.x & 63;
    const uint32_t v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;
    const uint64_t e0 = colptr[v], e1 = colptr[v + 1];
    float sv = 0.f;
    if (e1 > e0) sv = (azrow ? azrow[v] : az[e0]) > 0.f ? 1.f : 0.01f;
    const float *gr = grad + (size_t)v * ldg;
    float s = 0.f;
    for (uint32_t j = lane; j < F; j += 64) s = fmaf(gr[j] * sv, a[j], s);
    s = wave_sum(s);
    if (dA)
        for (uint64_t e = e0 + lane; e < e1; e += 64) dA[e] = s;
    if (lane == 0) {
        cw[v] = (float)(e1 - e0) * sv;
        drow[v] = s;
    }
}

hipError_t launch_edge_backward_gat(uint32_t N, uint32_t F, const uint64_t *colptr, const float *grad,
                                    uint32_t ldg, const float *az, const float *a, float *dA, float *cw,
                                    float *drow, hipStream_t s, const float *azrow) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(edge_backward_gat_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, F, colptr, grad,
                       ldg, az, a, dA, cw, drow, azrow);
    return hipGetLastError();
}

// y[v] = X[v,:] . r   (wave per row)
__global__ __launch_bounds__(256) void rowdot_kernel(uint32_t N, uint32_t F, const float *X, uint32_t ld,
                                                     const float *r, float *y) {
    const int lane = threadIdx.x & 63;
    const uint32_t v = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (v >= N) return;
    const float *xr = X + (size_t)v * ld;
    float s = 0.f;
    for (uint32_t j = lane; j < F; j += 64) s = fmaf(xr[j], r[j], s);
    s = wave_sum(s);
    if (lane == 0) y[v] = s;
}

// partial[b][j] = sum_{v in block b's rows} w[v] * X[v,j];  then out[j] = sum_b partial[b][j]
// out[j] = sum_v w[v] * X[v, j]: column sums weighted per row (the a_i gradient of the GAT prototype, CPU_comm.cpp:232-236).
// Round 6: float4 columns x row groups per workgroup (all 256 threads load, rows in flight in parallel) and a tree-free, fixed-order
// second stage on 32 columns x 8 row groups per workgroup -- 80 + 43 us -> per call at Reddit size before (one thread per column
// walking its block's rows, then one thread per column walking 1 024 partials).  Sums are formed in a fixed order: deterministic.
__global__ __launch_bounds__(256) void colsum_w_kernel(uint32_t N, uint32_t F, const float *X, uint32_t ld,
                                                       const float *w, float *partial, uint32_t rows_per_block) {
    __shared__ float4 red[256];
    const uint32_t r0 = blockIdx.x * rows_per_block;
    const uint32_t r1 = min(N, r0 + rows_per_block);
    const uint32_t F4 = (F + 3) >> 2;                 // float4 columns (rows are padded to 32 floats: the last one reads padding zeros)
    const uint32_t CW = min(F4, 256u);                // columns handled per pass
    const uint32_t RG = 256u / CW;                    // row groups
    const uint32_t c = threadIdx.x % CW, rg = threadIdx.x / CW;
    for (uint32_t c0 = 0; c0 < F4; c0 += CW) {
        const uint32_t col = c0 + c;
        float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
        if (col < F4 && rg < RG)
            for (uint32_t v = r0 + rg; v < r1; v += RG) {
                const float wv = w[v];
                float4 x;
                if ((ld & 3u) == 0) {
                    x = *reinterpret_cast<const float4 *>(X + (size_t)v * ld + 4 * col);
                } else {                               // (one-column tensors keep ld = 1: element loads, zeros past F)
                    const float *xr = X + (size_t)v * ld + 4 * col;
                    x = make_float4(xr[0], 4 * col + 1 < F ? xr[1] : 0.f, 4 * col + 2 < F ? xr[2] : 0.f, 4 * col + 3 < F ? xr[3] : 0.f);
                }
                s.x = fmaf(wv, x.x, s.x); s.y = fmaf(wv, x.y, s.y); s.z = fmaf(wv, x.z, s.z); s.w = fmaf(wv, x.w, s.w);
            }
        red[threadIdx.x] = s;
        __syncthreads();
        if (rg == 0 && col < F4) {
            for (uint32_t k = 1; k < RG; ++k) {       // row groups in order
                const float4 t = red[k * CW + c];
                s.x += t.x; s.y += t.y; s.z += t.z; s.w += t.w;
            }
            float *p = partial + (size_t)blockIdx.x * F + 4 * col;
            const float r[4] = {s.x, s.y, s.z, s.w};
            for (uint32_t q = 0; q < 4 && 4 * col + q < F; ++q) p[q] = r[q];
        }
        __syncthreads();
    }
}
__global__ __launch_bounds__(256) void colsum_final_kernel(uint32_t F, const float *partial, uint32_t nb, float *out) {
    __shared__ float red[256];
    const uint32_t c = threadIdx.x & 31u, rg = threadIdx.x >> 5;      // 32 columns x 8 groups of partials
    const uint32_t j = blockIdx.x * 32u + c;
    float s = 0.f;
    if (j < F)
        for (uint32_t b = rg; b < nb; b += 8) s += partial[(size_t)b * F + j];
    red[threadIdx.x] = s;
    __syncthreads();
    if (rg == 0 && j < F) {
        for (uint32_t k = 1; k < 8; ++k) s += red[k * 32 + c];
        out[j] = s;
    }
}

hipError_t launch_rowdot(uint32_t N, uint32_t F, const float *X, uint32_t ld, const float *r, float *y,
                         hipStream_t s) {
    if (N == 0) return hipSuccess;
    hipLaunchKernelGGL(rowdot_kernel, dim3((N + 3) / 4), dim3(256), 0, s, N, F, X, ld, r, y);
    return hipGetLastError();
}

// out[F] = X^T w, X is N x F; partial must hold nb*F floats
hipError_t launch_colsum_w(uint32_t N, uint32_t F, const float *X, uint32_t ld, const float *w,
                           float *partial, size_t partial_bytes, float *out, hipStream_t s) {
    if (F == 0) return hipSuccess;
    uint32_t nb = 512;
    while (nb > 1 && (nb > N / 64 || (size_t)nb * F * sizeof(float) > partial_bytes)) nb >>= 1;   // >= 64 rows per block
    const uint32_t rpb = (N + nb - 1) / nb > 0 ? (N + nb - 1) / nb : 1;
    nb = (N + rpb - 1) / rpb;
    if (nb == 0) nb = 1;
    hipLaunchKernelGGL(colsum_w_kernel, dim3(nb), dim3(256), 0, s, N, F, X, ld, w, partial, rpb);
    hipLaunchKernelGGL(colsum_final_kernel, dim3((F + 31) / 32), dim3(256), 0, s, F, partial, nb, out);
    return hipGetLastError();
}

// ---- K6: halo pack / unpack ------------------------------------------------------------
// pack:   dst[i, 0:cols] (dense) = src[rows[i], 0:cols]   (Engine::verticesPushOut's
//         memcpy loop, engine/utils.cpp:640-648, minus the 4-byte gvid per row)
// unpack: dst[rows[i], 0:cols] = src[i, 0:cols] (dense)   (ghostReceiverGCN's memcpy
//         loop at globalToGhostVtcs[gvid] - localVtxCnt, gcn_ops.cpp:310-318)
// cols is a multiple of 4 floats wherever ld is (pack buffers use the padded width).
__global__ void gather_rows_kernel(float *dst, const float *src, uint32_t ld, uint32_t cols4,
                                   const uint32_t *rows, uint32_t n) {
    const uint64_t total = (uint64_t)n * cols4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / cols4);
        const uint32_t c = (uint32_t)(i % cols4);
        reinterpret_cast<float4 *>(dst)[i] =
            reinterpret_cast<const float4 *>(src + (size_t)rows[r] * ld)[c];
    }
}
__global__ void scatter_rows_kernel(float *dst, const float *src, uint32_t ld, uint32_t cols4,
                                    const uint32_t *rows, uint32_t n) {
    const uint64_t total = (uint64_t)n * cols4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / cols4);
        const uint32_t c = (uint32_t)(i % cols4);
        reinterpret_cast<float4 *>(dst + (size_t)rows[r] * ld)[c] =
            reinterpret_cast<const float4 *>(src)[i];
    }
}

hipError_t launch_gather_rows(float *dst, const float *src, uint32_t ld, uint32_t cols,
                              const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || cols == 0) return hipSuccess;
    if ((cols & 3) || (ld & 3)) return hipErrorInvalidValue;   // float4 rows only (every exchanged tensor is padded to 32 floats)
    const uint64_t total = (uint64_t)n * (cols / 4);
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(gather_rows_kernel, dim3(blocks), dim3(256), 0, s, dst, src, ld, cols / 4, rows, n);
    return hipGetLastError();
}
hipError_t launch_scatter_rows(float *dst, const float *src, uint32_t ld, uint32_t cols,
                               const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || cols == 0) return hipSuccess;
    if ((cols & 3) || (ld & 3)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n * (cols / 4);
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(scatter_rows_kernel, dim3(blocks), dim3(256), 0, s, dst, src, ld, cols / 4, rows, n);
    return hipGetLastError();
}

// ---- K6, exact-width rows (option halo_exact_rows) ----------------------------------------
// The dense side holds rows of exactly `cols` floats, cols % 4 != 0: a dense row starts on a 4-byte boundary only, so the dense
// buffer is treated as ONE stream of n x cols floats and a thread owns one 16-byte-aligned quad of it.  A quad may straddle two
// rows (three and more when cols < 4): the thread resolves (row, col) of its first float once and walks the four elements with
// a carry.  A workgroup takes a run of `rpb` rows (a multiple of 4, so that the run starts on a 16-byte boundary of the
// stream; rpb x cols < 2^32): every index inside the run is 32-bit, one 32-bit divide per quad, no 64-bit divide.  The dense
// side moves as one 16-byte access per thread, the padded side as dwords (consecutive lanes, consecutive addresses within a
// row).  Only the stream's last quad can be partial (n x cols % 4 != 0): it moves as dwords -- not one float beyond n x cols
// is read or written on the dense side, the caller's buffer ends there.
// pack: the row list may repeat a row (a vertex goes to several peers).
__global__ __launch_bounds__(256) void gather_rows_exact_kernel(float *dst, const float *src, uint32_t ld, uint32_t cols,
                                                                const uint32_t *rows, uint32_t n, uint32_t rpb) {
    const uint32_t r0 = blockIdx.x * rpb;
    const uint32_t nr = n - r0 < rpb ? n - r0 : rpb;
    const uint32_t total = nr * cols;
    float *d = dst + (size_t)r0 * cols;
    const uint32_t *rw = rows + r0;
    for (uint32_t f = threadIdx.x * 4u; f < total; f += 1024u) {
        uint32_t r = f / cols, c = f - r * cols;
        const float *p = src + (size_t)rw[r] * ld;
        const uint32_t k_end = total - f < 4u ? total - f : 4u;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (k < k_end) {
                v[k] = p[c];
                if (++c == cols) {
                    c = 0;
                    if (++r < nr) p = src + (size_t)rw[r] * ld;
                }
            }
        }
        if (k_end == 4u) {
            *reinterpret_cast<float4 *>(d + f) = make_float4(v[0], v[1], v[2], v[3]);
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
                if (k < k_end) d[f + k] = v[k];
        }
    }
}
// unpack: the row list is a permutation of the ghost slots.  Writes [0, cols) of every listed row from the stream and zeros
// into [cols, ld): the raw ld-wide ghost rows are the bits the padded form leaves (the owner's zero padding travelled there).
__global__ __launch_bounds__(256) void scatter_rows_exact_kernel(float *dst, const float *src, uint32_t ld, uint32_t cols,
                                                                 const uint32_t *rows, uint32_t n, uint32_t rpb) {
    const uint32_t r0 = blockIdx.x * rpb;
    const uint32_t nr = n - r0 < rpb ? n - r0 : rpb;
    const uint32_t total = nr * cols;
    const float *s = src + (size_t)r0 * cols;
    const uint32_t *rw = rows + r0;
    for (uint32_t f = threadIdx.x * 4u; f < total; f += 1024u) {
        uint32_t r = f / cols, c = f - r * cols;
        float *p = dst + (size_t)rw[r] * ld;
        const uint32_t k_end = total - f < 4u ? total - f : 4u;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (k_end == 4u) {
            const float4 q = *reinterpret_cast<const float4 *>(s + f);
            v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
        } else {
#pragma unroll
            for (uint32_t k = 0; k < 3; ++k)
                if (k < k_end) v[k] = s[f + k];
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            if (k < k_end) {
                p[c] = v[k];
                if (++c == cols) {
                    c = 0;
                    if (++r < nr) p = dst + (size_t)rw[r] * ld;
                }
            }
        }
    }
    const uint32_t pad = ld - cols, ptotal = nr * pad;   // (ld <= cols + 31: far below 2^32 for a run of rows)
    for (uint32_t i = threadIdx.x; i < ptotal; i += 256u) {
        const uint32_t r = i / pad, c = cols + (i - r * pad);
        dst[(size_t)rw[r] * ld + c] = 0.f;
    }
}
// the same zeros after scatter_rows_kernel has written an exact width that is a multiple of 4 (cols4 < ld4, float4 units)
__global__ __launch_bounds__(256) void zero_rows_pad_kernel(float *dst, uint32_t ld, uint32_t cols4, uint32_t pad4,
                                                            const uint32_t *rows, uint32_t n) {
    const uint64_t total = (uint64_t)n * pad4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / pad4);
        const uint32_t c = cols4 + (uint32_t)(i % pad4);
        reinterpret_cast<float4 *>(dst + (size_t)rows[r] * ld)[c] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
}

// rows per workgroup of the exact kernels: a multiple of 4 (see above) with about 4096 floats = four quads per thread
static bool exact_rows_per_block(uint32_t cols, uint32_t ld, uint32_t *rpb) {
    const uint32_t r = ((4096u + cols - 1) / cols + 3u) & ~3u;
    if ((uint64_t)r * ld >= (1ull << 32)) return false;   // (ld >= cols: covers the stream's and the padding's indices)
    *rpb = r;
    return true;
}
hipError_t launch_gather_rows_exact(float *dst, const float *src, uint32_t ld, uint32_t cols,
                                    const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || cols == 0) return hipSuccess;
    uint32_t rpb;
    if (cols > ld || ((uintptr_t)dst & 15) || !exact_rows_per_block(cols, ld, &rpb)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gather_rows_exact_kernel, dim3((n - 1) / rpb + 1), dim3(256), 0, s, dst, src, ld, cols, rows, n, rpb);
    return hipGetLastError();
}
hipError_t launch_scatter_rows_exact(float *dst, const float *src, uint32_t ld, uint32_t cols,
                                     const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || cols == 0) return hipSuccess;
    uint32_t rpb;
    if (cols > ld || ((uintptr_t)src & 15) || !exact_rows_per_block(cols, ld, &rpb)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(scatter_rows_exact_kernel, dim3((n - 1) / rpb + 1), dim3(256), 0, s, dst, src, ld, cols, rows, n, rpb);
    return hipGetLastError();
}
hipError_t launch_zero_rows_pad(float *dst, uint32_t ld, uint32_t cols, const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || cols >= ld) return hipSuccess;
    if ((cols & 3) || (ld & 3)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n * ((ld - cols) / 4);
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(zero_rows_pad_kernel, dim3(blocks), dim3(256), 0, s, dst, ld, cols / 4, (ld - cols) / 4, rows, n);
    return hipGetLastError();
}

// ---- K6, merged rows (dory_gatmh_bwd_merged_exchange) ----------------------------------------------------------------------------
// The dense side holds rows of wa4 + wb4 quads: [a[v, 0:wa) | b[v, 0:wb)], the multi-head GAT's [do | st].  Every width and ld is a
// multiple of 4 floats, so no quad straddles the two parts or two rows: a thread owns one 16-byte quad -- one 16-byte load, one
// 16-byte store, 32-bit divides only (a run of rows per workgroup would save nothing here: the row width is not a compile-time
// constant either way).  pack: the row list may repeat a row (a vertex goes to several peers).
__global__ __launch_bounds__(256) void gather_rows_pair_kernel(float4 *dst, const float *a, uint32_t lda, uint32_t wa4, const float *b,
                                                               uint32_t ldb, uint32_t wb4, const uint32_t *rows, uint32_t n) {
    const uint32_t r4 = wa4 + wb4;
    const uint64_t total = (uint64_t)n * r4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / r4), c = (uint32_t)(i - (uint64_t)r * r4);
        const size_t v = rows[r];
        dst[i] = c < wa4 ? reinterpret_cast<const float4 *>(a + v * lda)[c] : reinterpret_cast<const float4 *>(b + v * ldb)[c - wa4];
    }
}
// unpack: the row list is a permutation of the ghost slots.  A thread owns one quad of a WHOLE row of a or of b (lda4 + ldb4 quads
// per listed row): the stream's value below the wire's width, zeros behind it -- the raw ghost rows are the bits the two separate
// exchanges leave (the owner's zero padding travelled there, or the exact form's zeroing wrote it).
__global__ __launch_bounds__(256) void scatter_rows_pair_kernel(float *a, uint32_t lda4, uint32_t wa4, float *b, uint32_t ldb4, uint32_t wb4,
                                                                const float4 *src, const uint32_t *rows, uint32_t n) {
    const uint32_t t4 = lda4 + ldb4, r4 = wa4 + wb4;
    const uint64_t total = (uint64_t)n * t4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / t4), c = (uint32_t)(i - (uint64_t)r * t4);
        const size_t v = rows[r];
        const bool first = c < lda4;
        const uint32_t cc = first ? c : c - lda4;                  // the quad inside its tensor's row
        const bool on_wire = cc < (first ? wa4 : wb4);
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (on_wire) q = src[(uint64_t)r * r4 + (first ? cc : wa4 + cc)];
        float4 *row = first ? reinterpret_cast<float4 *>(a + v * lda4 * 4) : reinterpret_cast<float4 *>(b + v * ldb4 * 4);
        row[cc] = q;
    }
}
hipError_t launch_gather_rows_pair(float *dst, const float *a, uint32_t lda, uint32_t wa, const float *b, uint32_t ldb, uint32_t wb,
                                   const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || wa + wb == 0) return hipSuccess;
    if (((wa | wb | lda | ldb) & 3) || wa > lda || wb > ldb || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n * ((wa + wb) / 4);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(gather_rows_pair_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<float4 *>(dst), a, lda, wa / 4, b, ldb, wb / 4, rows, n);
    return hipGetLastError();
}
hipError_t launch_scatter_rows_pair(float *a, uint32_t lda, uint32_t wa, float *b, uint32_t ldb, uint32_t wb, const float *src,
                                    const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || lda + ldb == 0) return hipSuccess;
    if (((wa | wb | lda | ldb) & 3) || wa > lda || wb > ldb || ((uintptr_t)src & 15)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n * ((lda + ldb) / 4);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(scatter_rows_pair_kernel, dim3(blocks), dim3(256), 0, s, a, lda / 4, wa / 4, b, ldb / 4, wb / 4,
                       reinterpret_cast<const float4 *>(src), rows, n);
    return hipGetLastError();
}

// ---- K6, merged rows with a bf16 first part (dory_gatmh_halo_bf16) ------------------------------------------------------------------
// The dense side holds rows of wa8 + wb4 chunks of 16 bytes: [a[v, 0:wa) as bf16 | b[v, 0:wb) as fp32], wa = 8 x wa8 -- the multiple
// of 8 puts the second part on a 16-byte boundary, so no chunk straddles the two parts or two rows and a thread owns one chunk.  pack:
// in the first part two 16-byte loads, four pack_bf16x2 (round to nearest even, the conversion of every bf16 path) and one 16-byte
// store; in the second one 16-byte load and one store.  The columns of a behind its cols are the tensor's zero padding, as in the fp32
// form.  The row list may repeat a row.  `total` = rows x chunks of this launch is at most 2^31 (the launcher slices the rows), so the
// index and its one divide are 32-bit.
__global__ __launch_bounds__(256) void gather_rows_pair_bf16_kernel(uint4 *dst, const float *a, uint32_t lda, uint32_t wa8, const float *b,
                                                                    uint32_t ldb, uint32_t wb4, const uint32_t *rows, uint32_t total) {
    const uint32_t r16 = wa8 + wb4, stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t r = i / r16, c = i - r * r16;
        const size_t v = rows[r];
        uint4 q;
        if (c < wa8) {
            const float4 *p = reinterpret_cast<const float4 *>(a + v * lda) + 2u * c;
            const float4 lo = p[0], hi = p[1];
            q = make_uint4(pack_bf16x2(lo.x, lo.y), pack_bf16x2(lo.z, lo.w), pack_bf16x2(hi.x, hi.y), pack_bf16x2(hi.z, hi.w));
        } else {
            q = reinterpret_cast<const uint4 *>(b + v * ldb)[c - wa8];
        }
        dst[i] = q;
    }
}
// unpack: a thread owns one quad of a WHOLE row of a or of b (lda4 + ldb4 quads per listed row), as the fp32 form's: below the wire's
// width four bf16 of the stream widened (a bf16 is the high half of the fp32 with the same value; 8-byte load) or one fp32 quad
// (16-byte load), zeros behind it.  `total` = rows x (lda4 + ldb4) of this launch is at most 2^31.
__global__ __launch_bounds__(256) void scatter_rows_pair_bf16_kernel(float *a, uint32_t lda4, uint32_t wa4, float *b, uint32_t ldb4, uint32_t wb4,
                                                                     const uint4 *src, const uint32_t *rows, uint32_t total) {
    const uint32_t t4 = lda4 + ldb4, wa8 = wa4 >> 1, r16 = wa8 + wb4, stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t r = i / t4, c = i - r * t4;
        const size_t v = rows[r];
        const bool first = c < lda4;
        const uint32_t cc = first ? c : c - lda4;                  // the quad inside its tensor's row
        float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
        if (first && cc < wa4) {
            const uint2 u = reinterpret_cast<const uint2 *>(src + (size_t)r * r16)[cc];
            q = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                            __uint_as_float(u.y & 0xFFFF0000u));
        } else if (!first && cc < wb4) {
            const uint4 u = src[(size_t)r * r16 + wa8 + cc];
            q = make_float4(__uint_as_float(u.x), __uint_as_float(u.y), __uint_as_float(u.z), __uint_as_float(u.w));
        }
        float4 *row = first ? reinterpret_cast<float4 *>(a + v * lda4 * 4) : reinterpret_cast<float4 *>(b + v * ldb4 * 4);
        row[cc] = q;
    }
}
// keep (dory_gatmh_bf16_ghosts): the first part stays bf16, in the row of a's bf16 twin (a16: lda8 chunks of 16 bytes a row) -- a thread owns
// one 16-byte chunk of a twin row (below the wire's width the stream's chunk as it is, zeros behind it: the bits rounding the fp32 row
// the kernel above leaves would give, whatever the twin held) or one quad of a whole row of b, as above.  `total` = rows x (lda8 + ldb4)
// of this launch is at most 2^31.
__global__ __launch_bounds__(256) void scatter_rows_pair_bf16_keep_kernel(uint16_t *a16, uint32_t lda8, uint32_t wa8, float *b, uint32_t ldb4,
                                                                          uint32_t wb4, const uint4 *src, const uint32_t *rows, uint32_t total) {
    const uint32_t t16 = lda8 + ldb4, r16 = wa8 + wb4, stride = gridDim.x * blockDim.x;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += stride) {
        const uint32_t r = i / t16, c = i - r * t16;
        const size_t v = rows[r];
        const bool first = c < lda8;
        const uint32_t cc = first ? c : c - lda8;                  // the chunk inside its tensor's row
        uint4 q = make_uint4(0u, 0u, 0u, 0u);
        if (cc < (first ? wa8 : wb4)) q = src[(size_t)r * r16 + (first ? cc : wa8 + cc)];
        uint4 *row = first ? reinterpret_cast<uint4 *>(a16 + v * lda8 * 8) : reinterpret_cast<uint4 *>(b + v * ldb4 * 4);
        row[cc] = q;
    }
}
// (rows per launch: rows x per_row <= 2^31, so that the kernels' indices stay 32-bit)
static uint32_t pair_bf16_rows_per_launch(uint32_t per_row) { return (1u << 31) / per_row; }
hipError_t launch_gather_rows_pair_bf16(float *dst, const float *a, uint32_t lda, uint32_t wa, const float *b, uint32_t ldb, uint32_t wb,
                                        const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || wa + wb == 0) return hipSuccess;
    if ((wa & 7) || ((wb | lda | ldb) & 3) || wa > lda || wb > ldb || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    const uint32_t r16 = wa / 8 + wb / 4, step = pair_bf16_rows_per_launch(r16);
    for (uint32_t r0 = 0; r0 < n; r0 += std::min(step, n - r0)) {
        const uint32_t total = std::min(step, n - r0) * r16;
        const uint32_t blocks = std::min<uint32_t>(2048u, (total + 255u) / 256u);
        hipLaunchKernelGGL(gather_rows_pair_bf16_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint4 *>(dst) + (size_t)r0 * r16, a, lda, wa / 8,
                           b, ldb, wb / 4, rows + r0, total);
    }
    return hipGetLastError();
}
hipError_t launch_scatter_rows_pair_bf16(float *a, uint32_t lda, uint32_t wa, float *b, uint32_t ldb, uint32_t wb, const float *src,
                                         const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || lda + ldb == 0) return hipSuccess;
    if ((wa & 7) || ((wb | lda | ldb) & 3) || wa > lda || wb > ldb || ((uintptr_t)src & 15)) return hipErrorInvalidValue;
    const uint32_t t4 = (lda + ldb) / 4, r16 = wa / 8 + wb / 4, step = pair_bf16_rows_per_launch(t4);
    for (uint32_t r0 = 0; r0 < n; r0 += std::min(step, n - r0)) {
        const uint32_t total = std::min(step, n - r0) * t4;
        const uint32_t blocks = std::min<uint32_t>(2048u, (total + 255u) / 256u);
        hipLaunchKernelGGL(scatter_rows_pair_bf16_kernel, dim3(blocks), dim3(256), 0, s, a, lda / 4, wa / 4, b, ldb / 4, wb / 4,
                           reinterpret_cast<const uint4 *>(src) + (size_t)r0 * r16, rows + r0, total);
    }
    return hipGetLastError();
}
hipError_t launch_scatter_rows_pair_bf16_keep(uint16_t *a16, uint32_t lda, uint32_t wa, float *b, uint32_t ldb, uint32_t wb, const float *src,
                                              const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || lda + ldb == 0) return hipSuccess;
    if (((wa | lda) & 7) || ((wb | ldb) & 3) || wa > lda || wb > ldb || (((uintptr_t)src | (uintptr_t)a16 | (uintptr_t)b) & 15)) return hipErrorInvalidValue;
    const uint32_t t16 = lda / 8 + ldb / 4, r16 = wa / 8 + wb / 4, step = pair_bf16_rows_per_launch(t16);
    for (uint32_t r0 = 0; r0 < n; r0 += std::min(step, n - r0)) {
        const uint32_t total = std::min(step, n - r0) * t16;
        const uint32_t blocks = std::min<uint32_t>(2048u, (total + 255u) / 256u);
        hipLaunchKernelGGL(scatter_rows_pair_bf16_keep_kernel, dim3(blocks), dim3(256), 0, s, a16, lda / 8, wa / 8, b, ldb / 4, wb / 4,
                           reinterpret_cast<const uint4 *>(src) + (size_t)r0 * r16, rows + r0, total);
    }
    return hipGetLastError();
}

// ---- K6, bf16 rows (dory_halo_bf16_rows) ----------------------------------------------------------------------------------------
// The dense side holds rows of `re4` quads of bf16 (row_elems = 4 x re4 elements, 8 bytes a quad): a row is a multiple of 8
// bytes, so no quad straddles two rows and a lane owns one quad of one row -- four elements per lane: one 16-byte load (or
// store) on the fp32 side, one 8-byte store (or load) on the dense side.  VEC: the tensor's ld is a multiple of 4 (every
// exchanged tensor but the one-column ones, ld == 1: those move as dwords on the fp32 side).
// pack: rounds with pack_bf16x2, the conversion of bf16_rows_kernel -- the bits the consumer's own rounding would give.
// Columns >= cols are never read: they are zeros on the dense side (padded form: cols == ld, the owner's padding travels as in
// the fp32 form).  The row list may repeat a row.
template <bool VEC>
__global__ __launch_bounds__(256) void gather_rows_bf16_kernel(uint2 *dst, const float *src, uint32_t ld, uint32_t cols, uint32_t re4,
                                                               const uint32_t *rows, uint32_t n) {
    const uint64_t total = (uint64_t)n * re4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / re4);
        const uint32_t c0 = (uint32_t)(i % re4) * 4u;
        const float *p = src + (size_t)rows[r] * ld;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c0 < cols) {
            if (VEC) {   // (c0 < cols <= ld, both multiples of 4 apart from cols: the quad lies inside the row)
                const float4 q = *reinterpret_cast<const float4 *>(p + c0);
                v[0] = q.x;
                v[1] = c0 + 1 < cols ? q.y : 0.f;
                v[2] = c0 + 2 < cols ? q.z : 0.f;
                v[3] = c0 + 3 < cols ? q.w : 0.f;
            } else {
#pragma unroll
                for (uint32_t k = 0; k < 4; ++k)
                    if (c0 + k < cols) v[k] = p[c0 + k];
            }
        }
        dst[i] = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}
// unpack: writes the whole ld-wide row of every listed ghost slot -- quads below re4 widened from the stream (a bf16 is the
// high half of the fp32 with the same value), zeros behind them: the bits the fp32 forms leave, whatever the padding held.
template <bool VEC>
__global__ __launch_bounds__(256) void scatter_rows_bf16_kernel(float *dst, const uint2 *src, uint32_t ld, uint32_t re4,
                                                                const uint32_t *rows, uint32_t n) {
    const uint32_t ld4 = (ld + 3u) >> 2;
    const uint64_t total = (uint64_t)n * ld4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / ld4);
        const uint32_t q = (uint32_t)(i % ld4);
        float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
        if (q < re4) {
            const uint2 u = src[(uint64_t)r * re4 + q];
            v = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                            __uint_as_float(u.y & 0xFFFF0000u));
        }
        float *p = dst + (size_t)rows[r] * ld;
        if (VEC) {
            reinterpret_cast<float4 *>(p)[q] = v;
        } else {
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t k = 0; k < 4; ++k)
                if (q * 4u + k < ld) p[q * 4u + k] = e[k];
        }
    }
}

hipError_t launch_gather_rows_bf16(void *dst, const float *src, uint32_t ld, uint32_t cols, uint32_t row_elems,
                                   const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || row_elems == 0) return hipSuccess;
    if ((row_elems & 3) || cols > ld || cols > row_elems || ((uintptr_t)dst & 7)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n * (row_elems / 4);
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    if (ld & 3) hipLaunchKernelGGL(gather_rows_bf16_kernel<false>, dim3(blocks), dim3(256), 0, s, static_cast<uint2 *>(dst), src, ld, cols, row_elems / 4, rows, n);
    else hipLaunchKernelGGL(gather_rows_bf16_kernel<true>, dim3(blocks), dim3(256), 0, s, static_cast<uint2 *>(dst), src, ld, cols, row_elems / 4, rows, n);
    return hipGetLastError();
}
hipError_t launch_scatter_rows_bf16(float *dst, const void *src, uint32_t ld, uint32_t row_elems,
                                    const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || ld == 0) return hipSuccess;
    if ((row_elems & 3) || row_elems > ((ld + 3u) & ~3u) || ((uintptr_t)src & 7)) return hipErrorInvalidValue;
    const uint64_t total = (uint64_t)n * ((ld + 3u) / 4);
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    if (ld & 3) hipLaunchKernelGGL(scatter_rows_bf16_kernel<false>, dim3(blocks), dim3(256), 0, s, dst, static_cast<const uint2 *>(src), ld, row_elems / 4, rows, n);
    else hipLaunchKernelGGL(scatter_rows_bf16_kernel<true>, dim3(blocks), dim3(256), 0, s, dst, static_cast<const uint2 *>(src), ld, row_elems / 4, rows, n);
    return hipGetLastError();
}

// ---- K6, bf16 ghost twins (dory_halo_bf16_ghosts) --------------------------------------------------------------------------------
// keep: the received bf16 rows stay bf16 -- row r of the stream (re4 quads of 8 bytes) goes to row rows[r] of the twin (stride ld, a
// multiple of 32 elements: rows of whole 64 bytes, 16-byte aligned), zeros in [4 x re4, ld): the bits rounding the fp32 row that
// scatter_rows_bf16_kernel leaves would give (widening and rounding a bf16 cancel), whatever the twin held before.  A lane owns LE
// elements of a twin row.  LE == 8: one 16-byte chunk, filled from two 8-byte quads of the stream (rows of the stream are 8-byte
// aligned only), either of which may lie behind the stream's row; one 16-byte store.  LE == 4: one quad, one 8-byte load (or zeros),
// one 8-byte store.  The launcher instantiates LE == 4: measured 4-10 % faster than LE == 8 at every shape (3.15 M rows; stand-alone
// copies of both in tools/probes/halo_bf16_keep_forms.hip, numbers in profiles/HISTORY.md section 21) -- as with the widening unpack.
template <int LE>
__global__ __launch_bounds__(256) void scatter_rows_bf16_keep_kernel(uint16_t *dst, const uint2 *src, uint32_t ld, uint32_t re4,
                                                                     const uint32_t *rows, uint32_t n) {
    static_assert(LE == 4 || LE == 8, "a lane owns one 8-byte quad or one 16-byte chunk");
    const uint32_t per_row = ld / LE;
    const uint64_t total = (uint64_t)n * per_row;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / per_row);
        const uint32_t k = (uint32_t)(i % per_row);
        const uint2 *in = src + (uint64_t)r * re4;
        uint16_t *out = dst + (size_t)rows[r] * ld;
        if (LE == 8) {
            const uint32_t q = 2u * k;
            const uint2 a = q < re4 ? in[q] : make_uint2(0u, 0u);
            const uint2 b = q + 1u < re4 ? in[q + 1u] : make_uint2(0u, 0u);
            reinterpret_cast<uint4 *>(out)[k] = make_uint4(a.x, a.y, b.x, b.y);
        } else {
            reinterpret_cast<uint2 *>(out)[k] = k < re4 ? in[k] : make_uint2(0u, 0u);
        }
    }
}
// widen: a whole twin into its fp32 tensor, dense (row r to row r, every one of the ld elements): a lane reads 8 bf16 (16 bytes) and
// stores two float4 -- a bf16 is the high half of the fp32 with the same value
__global__ __launch_bounds__(256) void widen_rows_bf16_kernel(float4 *dst, const uint4 *src, uint64_t n8) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n8; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint4 u = src[i];
        dst[2 * i] = make_float4(__uint_as_float(u.x << 16), __uint_as_float(u.x & 0xFFFF0000u), __uint_as_float(u.y << 16),
                                 __uint_as_float(u.y & 0xFFFF0000u));
        dst[2 * i + 1] = make_float4(__uint_as_float(u.z << 16), __uint_as_float(u.z & 0xFFFF0000u), __uint_as_float(u.w << 16),
                                     __uint_as_float(u.w & 0xFFFF0000u));
    }
}

hipError_t launch_scatter_rows_bf16_keep(uint16_t *dst, const void *src, uint32_t ld, uint32_t row_elems,
                                         const uint32_t *rows, uint32_t n, hipStream_t s) {
    if (n == 0 || ld == 0) return hipSuccess;
    if ((ld & 31) || (row_elems & 3) || row_elems > ld || ((uintptr_t)src & 7) || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    constexpr int LE = 4;   // (the lane form in use: the faster of the two)
    const uint64_t total = (uint64_t)n * (ld / LE);
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(scatter_rows_bf16_keep_kernel<LE>, dim3(blocks), dim3(256), 0, s, dst, static_cast<const uint2 *>(src), ld, row_elems / 4, rows, n);
    return hipGetLastError();
}
hipError_t launch_widen_rows_bf16(float *dst, const uint16_t *src, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if ((n & 7) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return hipErrorInvalidValue;
    const uint64_t n8 = n / 8;
    hipLaunchKernelGGL(widen_rows_bf16_kernel, dim3((uint32_t)std::min<uint64_t>(8192, (n8 + 255) / 256)), dim3(256), 0, s,
                       reinterpret_cast<float4 *>(dst), reinterpret_cast<const uint4 *>(src), n8);
    return hipGetLastError();
}

// ---- option halo_direct_recv: a ghost tensor between its caller-visible and its stored (wire) order ------------------------
// Whole ld-wide rows, a dword per thread (ld may be 1: the per-head tensors of a single head), `order` a permutation of
// [0, n).  Off the epoch's path: dory_tensor_upload / dory_tensor_download of a ghost tensor only.
__global__ __launch_bounds__(256) void permute_rows_kernel(float *dst, const float *src, uint32_t ld, const uint32_t *order,
                                                           uint32_t n, int to_wire) {
    const uint64_t total = (uint64_t)n * ld;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / ld);
        const uint32_t c = (uint32_t)(i - (uint64_t)r * ld);
        const size_t other = (size_t)order[r] * ld + c;
        if (to_wire) dst[i] = src[other];
        else dst[other] = src[i];
    }
}
hipError_t launch_permute_rows(float *dst, const float *src, uint32_t ld, const uint32_t *order, uint32_t n, bool to_wire, hipStream_t s) {
    if (n == 0 || ld == 0) return hipSuccess;
    const uint64_t total = (uint64_t)n * ld;
    int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    hipLaunchKernelGGL(permute_rows_kernel, dim3(blocks), dim3(256), 0, s, dst, src, ld, order, n, to_wire ? 1 : 0);
    return hipGetLastError();
}

// ---- K6, scatter messages (dory_scatter_msgs_*: the reference's own wire, include/dorylus_wire.h) ---------------------------
// A message is 7 header dwords and then records of 1 + F dwords (global vertex id, F floats): every row sits at a one-dword
// skew against the last one, whatever F is.  Both kernels stage through LDS, which absorbs that skew: the tensor side moves as
// 16-byte accesses of whole rows (rows start on 128-byte lines; tensors with ld % 4 != 0 -- ld == 1 -- move as dwords), the
// message side as 16-byte accesses of the message's own quads (messages start 16-byte aligned), and only LDS is addressed dword
// by dword.  Indices inside a workgroup's piece are 32-bit; the piece's base is the only 64-bit value.
__device__ __forceinline__ uint32_t scatter_hex8_word(uint32_t receiver, uint32_t w) {   // characters 4w .. 4w + 3 of sprintf("%8X")
    uint32_t out = 0;
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
        const uint32_t j = 4 * w + k, rest = receiver >> (4 * (7 - j)), d = rest & 15u;
        const uint32_t ch = (rest == 0 && j != 7) ? 0x20u : (d < 10 ? 0x30u + d : 0x41u + d - 10u);
        out |= ch << (8 * k);
    }
    return out;
}
// pack: a workgroup writes SCATTER_PACK_DW consecutive dwords [lo, hi) of one message -- whole quads, but for the message's last
// dwords -- after gathering what falls into them: header words, ids (l2g[lvid]) and the columns [0, F) of the listed rows (a
// record cut by lo or hi is loaded by both neighbours, each keeping its own part; a float4 wholly outside is not loaded).  The
// padding columns of a source row may be read into registers and are never stored.  The send list may repeat a row.  Behind a
// message that is not the last one, the dwords up to the next 16-byte boundary are written as zeros.
constexpr uint32_t SCATTER_PACK_DW = 4096;
template <bool VEC>
__global__ __launch_bounds__(256) void scatter_msgs_pack_kernel(uint32_t *buf, const float *src, uint32_t ld, uint32_t F, const uint32_t *lvids,
                                                                const uint32_t *l2g, const dory_scatter_msg *msgs, uint32_t n_msgs,
                                                                uint32_t chunks_per_msg, uint32_t sender, uint32_t layer, uint32_t dir) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[SCATTER_PACK_DW];
    const uint32_t m = blockIdx.x / chunks_per_msg, k = blockIdx.x - m * chunks_per_msg;
    const dory_scatter_msg M = msgs[m];
    const uint32_t rec = 1u + F, msg_dw = 7u + M.rows * rec, lo = k * SCATTER_PACK_DW;
    if (lo >= msg_dw) return;
    const uint32_t hi = msg_dw - lo < SCATTER_PACK_DW ? msg_dw : lo + SCATTER_PACK_DW, n = hi - lo;
    if (lo == 0 && threadIdx.x < 7) {
        const uint32_t t = threadIdx.x;
        stage[t] = t < 2 ? scatter_hex8_word(M.peer, t) : t == 2 ? sender : t == 3 ? M.rows : t == 4 ? F : t == 5 ? layer : dir;
    }
    const uint32_t r_lo = lo > 7u ? (lo - 7u) / rec : 0u, r_hi = (hi - 7u + rec - 1u) / rec, nr = r_hi - r_lo;   // (hi > 7: a message has a record)
    const uint32_t *lv = lvids + M.first_row + r_lo;
    const int32_t b0 = (int32_t)(7u + r_lo * rec) - (int32_t)lo;   // where record r_lo starts in `stage` (may lie in front of it)
    for (uint32_t r = threadIdx.x; r < nr; r += 256u) {
        const uint32_t p = (uint32_t)(b0 + (int32_t)(r * rec));
        if (p < n) stage[p] = l2g[lv[r]];
    }
    if (VEC) {
        const uint32_t F4 = (F + 3u) >> 2;
        for (uint32_t i = threadIdx.x; i < nr * F4; i += 256u) {
            const uint32_t r = i / F4, c = (i - r * F4) * 4u;
            const int32_t p0 = b0 + (int32_t)(r * rec + 1u + c);
            if (p0 + 4 <= 0 || p0 >= (int32_t)n) continue;
            const uint4 v = *reinterpret_cast<const uint4 *>(src + (size_t)lv[r] * ld + c);
            const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (uint32_t e = 0; e < 4; ++e)
                if (c + e < F && (uint32_t)(p0 + (int32_t)e) < n) stage[p0 + (int32_t)e] = w[e];
        }
    } else {
        for (uint32_t i = threadIdx.x; i < nr * F; i += 256u) {
            const uint32_t r = i / F, c = i - r * F, p = (uint32_t)(b0 + (int32_t)(r * rec + 1u + c));
            if (p < n) stage[p] = __float_as_uint(src[(size_t)lv[r] * ld + c]);
        }
    }
    __syncthreads();
    uint32_t *out = buf + (M.offset >> 2) + lo;
    const uint32_t nq = n >> 2, tail = n & 3u;
    for (uint32_t q = threadIdx.x; q < nq; q += 256u)
        *reinterpret_cast<uint4 *>(out + 4u * q) = *reinterpret_cast<const uint4 *>(stage + 4u * q);
    if (tail && threadIdx.x < 4u) {   // the message's last dwords, and the zeros between it and the next message
        if (threadIdx.x < tail) out[4u * nq + threadIdx.x] = stage[4u * nq + threadIdx.x];
        else if (m + 1u < n_msgs) out[4u * nq + threadIdx.x] = 0u;
    }
}
// unpack: a workgroup takes a run of `rpb` WHOLE records of a stream of records (a message's payload: no header), loads the quads
// that cover them into LDS (a quad shared with the neighbour run is read by both; the stream's last dwords move as dwords), finds
// every record's ghost slot by binary search of the ascending id table, claims the slot for this round (atomic exchange of its
// stamp: an id that is not in the table, or whose slot carries this round's stamp already, is counted and never written), maps
// the slot to its stored row (option halo_direct_recv: slot_row) and writes the whole ld-wide row: [0, F) from the record, zeros
// into [F, ld).  rpb x (1 + F) + 6 <= SCATTER_UNPACK_DW.
constexpr uint32_t SCATTER_UNPACK_DW = 8192;
template <bool VEC>
__global__ __launch_bounds__(256) void scatter_msgs_unpack_kernel(float *ghost, uint32_t ld, uint32_t F, const uint32_t *stream, uint32_t nrec,
                                                                  uint32_t rpb, const uint32_t *gvids, uint32_t G, const uint32_t *slot_row,
                                                                  uint32_t *stamp, uint32_t round, uint32_t *counts) {
    __shared__ __attribute__((aligned(16))) uint32_t stage[SCATTER_UNPACK_DW];
    __shared__ uint32_t cnt[3];
    const uint32_t rec = 1u + F, r0 = blockIdx.x * rpb, nr = nrec - r0 < rpb ? nrec - r0 : rpb;
    const uint64_t total = (uint64_t)nrec * rec, d_lo = (uint64_t)r0 * rec, a_lo = d_lo & ~3ull;
    const uint64_t d_hi = d_lo + (uint64_t)nr * rec, a_hi = ((d_hi + 3ull) & ~3ull) < total ? ((d_hi + 3ull) & ~3ull) : total;
    const uint32_t off = (uint32_t)(d_lo - a_lo), n = (uint32_t)(a_hi - a_lo), nq = n >> 2, tail = n & 3u;
    const uint32_t *in = stream + a_lo;
    if (threadIdx.x < 3) cnt[threadIdx.x] = 0;
    for (uint32_t q = threadIdx.x; q < nq; q += 256u)
        *reinterpret_cast<uint4 *>(stage + 4u * q) = *reinterpret_cast<const uint4 *>(in + 4u * q);
    if (threadIdx.x < tail) stage[4u * nq + threadIdx.x] = in[4u * nq + threadIdx.x];
    __syncthreads();
    for (uint32_t r = threadIdx.x; r < nr; r += 256u) {
        const uint32_t p = off + r * rec, gv = stage[p];
        uint32_t a = 0, b = G;
        while (a < b) {
            const uint32_t mid = (a + b) >> 1;
            if (gvids[mid] < gv) a = mid + 1u;
            else b = mid;
        }
        uint32_t row = 0xFFFFFFFFu;
        if (a >= G || gvids[a] != gv) {
            atomicAdd(&cnt[1], 1u);
        } else if (atomicExch(&stamp[a], round) == round) {
            atomicAdd(&cnt[2], 1u);
        } else {
            atomicAdd(&cnt[0], 1u);
            row = slot_row ? slot_row[a] : a;
        }
        stage[p] = row;
    }
    __syncthreads();
    if (threadIdx.x < 3 && cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], cnt[threadIdx.x]);
    if (VEC) {
        const uint32_t ld4 = ld >> 2;
        for (uint32_t i = threadIdx.x; i < nr * ld4; i += 256u) {
            const uint32_t r = i / ld4, c = (i - r * ld4) * 4u, p = off + r * rec, row = stage[p];
            if (row == 0xFFFFFFFFu) continue;
            uint4 v;
            v.x = c < F ? stage[p + 1u + c] : 0u;
            v.y = c + 1u < F ? stage[p + 2u + c] : 0u;
            v.z = c + 2u < F ? stage[p + 3u + c] : 0u;
            v.w = c + 3u < F ? stage[p + 4u + c] : 0u;
            *reinterpret_cast<uint4 *>(ghost + (size_t)row * ld + c) = v;
        }
    } else {
        for (uint32_t i = threadIdx.x; i < nr * ld; i += 256u) {
            const uint32_t r = i / ld, c = i - r * ld, p = off + r * rec, row = stage[p];
            if (row != 0xFFFFFFFFu) ghost[(size_t)row * ld + c] = c < F ? __uint_as_float(stage[p + 1u + c]) : 0.f;
        }
    }
}

uint32_t scatter_msgs_max_cols() { return SCATTER_UNPACK_DW - 7u; }
hipError_t launch_scatter_msgs_pack(void *buf, const float *src, uint32_t ld, uint32_t cols, const uint32_t *lvids, const uint32_t *l2g,
                                    const dory_scatter_msg *d_msgs, uint32_t n_msgs, uint32_t max_rows, uint32_t sender, uint32_t layer,
                                    uint32_t dir, hipStream_t s) {
    if (n_msgs == 0) return hipSuccess;
    const uint64_t msg_dw = 7ull + (uint64_t)max_rows * (1ull + cols);
    if (cols == 0 || cols > ld || max_rows == 0 || msg_dw >= (1ull << 30) || ((uintptr_t)buf & 15)) return hipErrorInvalidValue;
    const uint64_t cpm = (msg_dw + SCATTER_PACK_DW - 1) / SCATTER_PACK_DW, grid = cpm * n_msgs;
    if (grid >= (1ull << 31)) return hipErrorInvalidValue;
    const bool vec = (ld & 3u) == 0 && ((cols + 3u) & ~3u) <= ld && ((uintptr_t)src & 15) == 0;
    if (vec) hipLaunchKernelGGL(scatter_msgs_pack_kernel<true>, dim3((uint32_t)grid), dim3(256), 0, s, (uint32_t *)buf, src, ld, cols, lvids, l2g,
                                d_msgs, n_msgs, (uint32_t)cpm, sender, layer, dir);
    else hipLaunchKernelGGL(scatter_msgs_pack_kernel<false>, dim3((uint32_t)grid), dim3(256), 0, s, (uint32_t *)buf, src, ld, cols, lvids, l2g,
                            d_msgs, n_msgs, (uint32_t)cpm, sender, layer, dir);
    return hipGetLastError();
}
hipError_t launch_scatter_msgs_unpack(float *ghost, uint32_t ld, uint32_t cols, const void *records, uint32_t nrec, const uint32_t *gvids,
                                      uint32_t G, const uint32_t *slot_row, uint32_t *stamp, uint32_t round, uint32_t *counts, hipStream_t s) {
    if (nrec == 0) return hipSuccess;
    if (cols == 0 || cols > ld || cols > scatter_msgs_max_cols() || ((uintptr_t)records & 15)) return hipErrorInvalidValue;
    const uint32_t rpb = (SCATTER_UNPACK_DW - 6u) / (1u + cols);
    const uint32_t grid = (nrec - 1u) / rpb + 1u;
    const bool vec = (ld & 3u) == 0 && ((uintptr_t)ghost & 15) == 0;
    if (vec) hipLaunchKernelGGL(scatter_msgs_unpack_kernel<true>, dim3(grid), dim3(256), 0, s, ghost, ld, cols, (const uint32_t *)records, nrec, rpb,
                                gvids, G, slot_row, stamp, round, counts);
    else hipLaunchKernelGGL(scatter_msgs_unpack_kernel<false>, dim3(grid), dim3(256), 0, s, ghost, ld, cols, (const uint32_t *)records, nrec, rpb,
                            gvids, G, slot_row, stamp, round, counts);
    return hipGetLastError();
}

// ---- K7: Adam -----------------------------------------------------------------------------
// AdamOptimizer::update (reference src/weight-server/AdamOptimizer.cpp:36-51), the
// mixed float/double expressions kept as written there ("(1. - BETA1) * gt" is double).
__global__ void adam_kernel(float *w, const float *g, float *m, float *v, uint64_t n, float lr_t) {
    const float BETA1 = .9f, BETA2 = .999f, EPSILON = 1e-07f;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const float gt = g[i];
        const float pm = m[i], pd = v[i];
        const float nm = (float)(BETA1 * pm + (1. - BETA1) * gt);
        const float nv = (float)(BETA2 * pd + (1. - BETA2) * gt * gt);
        m[i] = nm;
        v[i] = nv;
        const float delta = (float)(lr_t * nm / (sqrt((double)nv) + EPSILON));
        w[i] -= delta;
    }
}

hipError_t launch_adam(float *w, const float *g, float *m, float *v, uint64_t n, float lr_t,
                       hipStream_t s) {
    if (n == 0) return hipSuccess;
    int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(adam_kernel, dim3(blocks), dim3(256), 0, s, w, g, m, v, n, lr_t);
    return hipGetLastError();
}

// the same update inside a replayed epoch graph: the step size of replay number *idx comes
// from a table the host filled before the launches (kernel arguments are frozen at capture)
__global__ void adam_table_kernel(float *w, const float *g, float *m, float *v, uint64_t n, const float *lr_table,
                                  const uint32_t *idx) {
    const float BETA1 = .9f, BETA2 = .999f, EPSILON = 1e-07f;
    const float lr_t = lr_table[*idx];
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n;
         i += (uint64_t)gridDim.x * blockDim.x) {
        const float gt = g[i];
        const float pm = m[i], pd = v[i];
        const float nm = (float)(BETA1 * pm + (1. - BETA1) * gt);
        const float nv = (float)(BETA2 * pd + (1. - BETA2) * gt * gt);
        m[i] = nm;
        v[i] = nv;
        const float delta = (float)(lr_t * nm / (sqrt((double)nv) + EPSILON));
        w[i] -= delta;
    }
}
__global__ void bump_counter_kernel(uint32_t *idx) { *idx += 1u; }

hipError_t launch_adam_table(float *w, const float *g, float *m, float *v, uint64_t n, const float *lr_table,
                             const uint32_t *idx, hipStream_t s) {
    if (n == 0) return hipSuccess;
    int blocks = (int)((n + 255) / 256 < 1024 ? (n + 255) / 256 : 1024);
    hipLaunchKernelGGL(adam_table_kernel, dim3(blocks), dim3(256), 0, s, w, g, m, v, n, lr_table, idx);
    return hipGetLastError();
}
hipError_t launch_bump_counter(uint32_t *idx, hipStream_t s) {
    hipLaunchKernelGGL(bump_counter_kernel, dim3(1), dim3(1), 0, s, idx);
    return hipGetLastError();
}

}  // namespace dory
