// gemm_send16_forms.hip -- the two epilogue forms of K2's bf16 send kernels (dory_halo_fused_pack_bf16; csrc/gemm.hip, included
// here: these are the library's own kernels, not copies) side by side, beside what they replace:
//   form 1  the neighbouring lane's value by DPP, the even lanes store one cvt_pk dword (the form the library instantiates)
//   form 2  every lane one 2-byte store
//   plain   the GEMM without a send form, then pack  = a stand-alone copy of gather_rows_bf16_kernel (csrc/elementwise.hip) over
//           its output: the pair the fused form replaces
//   fp32    the fp32 send kernel (dory_halo_fused_pack) for scale
// NN products M x 128 -> M x N, every row sent once (identity slots), rows padded (w = ld) and exact (w = cols rounded up to 4);
// 10 launches after a warm one, ROUNDS rounds alternating the forms; the two forms' buffers are compared byte for byte with the
// pack kernel's over the first rows.  The faster form is the one the library runs (profiles/r21_halo_fused_pack_bf16.txt).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probes/gemm_send16_forms.hip -o tools/probes/gemm_send16_forms
#include "../../dorylus_amd/csrc/gemm.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

#define CK(x)                                                                                   \
    do {                                                                                        \
        hipError_t e__ = (x);                                                                   \
        if (e__ != hipSuccess) {                                                                \
            fprintf(stderr, "%s failed: %s (line %d)\n", #x, hipGetErrorString(e__), __LINE__); \
            exit(1);                                                                            \
        }                                                                                       \
    } while (0)

using namespace dory;

// gather_rows_bf16_kernel<true> of csrc/elementwise.hip
__global__ __launch_bounds__(256) void pack16_kernel(uint2 *dst, const float *src, uint32_t ld, uint32_t cols, uint32_t re4, const uint32_t *rows, uint32_t n) {
    const uint64_t total = (uint64_t)n * re4;
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (uint64_t)gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t)(i / re4);
        const uint32_t c0 = (uint32_t)(i % re4) * 4u;
        const float *p = src + (size_t)rows[r] * ld;
        float v[4] = {0.f, 0.f, 0.f, 0.f};
        if (c0 < cols) {
            const float4 q = *reinterpret_cast<const float4 *>(p + c0);
            v[0] = q.x;
            v[1] = c0 + 1 < cols ? q.y : 0.f;
            v[2] = c0 + 2 < cols ? q.z : 0.f;
            v[3] = c0 + 3 < cols ? q.w : 0.f;
        }
        dst[i] = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

enum Form { PLAIN = 0, FP32 = 1, F1 = 2, F2 = 3, PACK = 4, NFORMS = 5 };
static const char *const NAMES[NFORMS] = {"plain GEMM", "fp32 send", "send16 form 1 (DPP pair)", "send16 form 2 (2-byte)", "bf16 pack kernel"};

static void launch(Form f, const GemmArgs &g, GemmSend sd, const uint32_t *ident) {
    const uint32_t klen = (g.K + 15u) / 16u * 16u;
    const dim3 block(256);
    if (f == PACK) {
        const uint64_t total = (uint64_t)g.M * (sd.w / 4);
        const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
        hipLaunchKernelGGL(pack16_kernel, dim3(blocks), block, 0, nullptr, reinterpret_cast<uint2 *>(sd.buf), g.C, g.ldc, g.N, sd.w / 4, ident, g.M);
        return;
    }
    if (g.N > 64) {
        const dim3 grid((g.M + 127) / 128, (g.N + 127) / 128, 1);
        if (f == PLAIN) hipLaunchKernelGGL((gemm_dma_kernel_occ4<128, 2, 2, 2, 2, false, true, 16>), grid, block, 0, nullptr, g, klen, (float *)nullptr);
        if (f == FP32) hipLaunchKernelGGL((gemm_dma_send_kernel_occ4<128, 2, 2, 2, 2, false, true, 16>), grid, block, 0, nullptr, g, klen, (float *)nullptr, sd);
        if (f == F1) hipLaunchKernelGGL((gemm_dma_send16_kernel_occ4<128, 2, 2, 2, 2, false, true, 16, 1>), grid, block, 0, nullptr, g, klen, (float *)nullptr, sd);
        if (f == F2) hipLaunchKernelGGL((gemm_dma_send16_kernel_occ4<128, 2, 2, 2, 2, false, true, 16, 2>), grid, block, 0, nullptr, g, klen, (float *)nullptr, sd);
    } else {
        const dim3 grid((g.M + 127) / 128, 1, 1);
        if (f == PLAIN) hipLaunchKernelGGL((gemm_dma_kernel<64, 4, 1, 1, 2, false, true, 16>), grid, block, 0, nullptr, g, klen, (float *)nullptr);
        if (f == FP32) hipLaunchKernelGGL((gemm_dma_send_kernel<64, 4, 1, 1, 2, false, true, 16>), grid, block, 0, nullptr, g, klen, (float *)nullptr, sd);
        if (f == F1) hipLaunchKernelGGL((gemm_dma_send16_kernel<64, 4, 1, 1, 2, false, true, 16, 1>), grid, block, 0, nullptr, g, klen, (float *)nullptr, sd);
        if (f == F2) hipLaunchKernelGGL((gemm_dma_send16_kernel<64, 4, 1, 1, 2, false, true, 16, 2>), grid, block, 0, nullptr, g, klen, (float *)nullptr, sd);
    }
}

static float timed(Form f, const GemmArgs &g, const GemmSend &sd, const uint32_t *ident, hipEvent_t a, hipEvent_t b) {
    for (int i = 0; i < 11; ++i) {
        if (i == 1) CK(hipEventRecord(a, nullptr));
        launch(f, g, sd, ident);
    }
    CK(hipGetLastError());
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / 10.f;
}

int main(int argc, char **argv) {
    const uint32_t M = argc > 1 ? (uint32_t)atoll(argv[1]) : 1u << 20;
    const int ROUNDS = argc > 2 ? atoi(argv[2]) : 3;
    const uint32_t K = 128;
    const uint32_t widths[] = {128, 64, 48, 41, 300};
    const uint32_t CHECK_ROWS = M < 4096 ? M : 4096;
    std::vector<uint32_t> map((size_t)2 * M + 1);
    std::iota(map.begin(), map.begin() + M + 1, 0u);          // row_ptr: every row one slot
    std::iota(map.begin() + M + 1, map.end(), 0u);            // row_slots: its own index
    uint32_t *d_map = nullptr;
    CK(hipMalloc((void **)&d_map, map.size() * 4));
    CK(hipMemcpy(d_map, map.data(), map.size() * 4, hipMemcpyHostToDevice));
    float *A = nullptr;
    CK(hipMalloc((void **)&A, (size_t)M * K * 4));
    {
        std::vector<float> h((size_t)M * K);
        uint32_t s = 12345u;
        for (auto &x : h) { s = s * 1664525u + 1013904223u; x = (float)(int32_t)(s >> 8) * (1.f / 8388608.f) - 1.f; }
        CK(hipMemcpy(A, h.data(), h.size() * 4, hipMemcpyHostToDevice));
    }
    hipEvent_t ea, eb;
    CK(hipEventCreate(&ea));
    CK(hipEventCreate(&eb));
    printf("# tools/probes/gemm_send16_forms: NN %u x %u -> N, every row sent once; ms per launch (mean of 10 after a warm one), %d rounds alternating\n", M, K, ROUNDS);
    printf("# N | w (bf16 elements a row) |");
    for (int f = 0; f < NFORMS; ++f) printf(" %s (rounds) |", NAMES[f]);
    printf(" medians: plain + pack | form 1 | form 2 | bytes equal\n");
    for (uint32_t N : widths) {
        const uint32_t ld = pad_ld(N);
        float *B = nullptr, *C = nullptr, *buf = nullptr;
        CK(hipMalloc((void **)&B, (size_t)K * ld * 4));
        CK(hipMalloc((void **)&C, (size_t)M * ld * 4));
        CK(hipMalloc((void **)&buf, (size_t)M * ld * 4));      // (room for fp32 rows)
        {
            std::vector<float> h((size_t)K * ld, 0.f);
            uint32_t s = 777u + N;
            for (uint32_t k = 0; k < K; ++k)
                for (uint32_t j = 0; j < N; ++j) { s = s * 1664525u + 1013904223u; h[(size_t)k * ld + j] = ((float)(int32_t)(s >> 8) * (1.f / 8388608.f) - 1.f) * 0.1f; }
            CK(hipMemcpy(B, h.data(), h.size() * 4, hipMemcpyHostToDevice));
        }
        CK(hipMemset(C, 0, (size_t)M * ld * 4));
        GemmArgs g{};
        g.M = M; g.N = N; g.K = K; g.A = A; g.lda = K; g.B = B; g.ldb = ld; g.C = C; g.ldc = ld; g.epilogue = EPI_NONE;
        for (int exact = 0; exact < 2; ++exact) {
            const uint32_t w = exact ? (N + 3u) & ~3u : ld;
            if (exact && w == ld) continue;
            GemmSend sd{};
            sd.buf = buf; sd.row_ptr = d_map; sd.row_slots = d_map + M + 1; sd.w = w; sd.which = 0; sd.cols = N; sd.bf16 = 1;
            GemmSend sd32 = sd;
            sd32.bf16 = 0;
            sd32.w = exact ? N : ld;
            // the bytes first: pack kernel over the plain product, then each form
            std::vector<uint16_t> want((size_t)CHECK_ROWS * w), got((size_t)CHECK_ROWS * w);
            launch(PLAIN, g, sd, d_map + M + 1);
            launch(PACK, g, sd, d_map + M + 1);
            CK(hipDeviceSynchronize());
            CK(hipMemcpy(want.data(), buf, want.size() * 2, hipMemcpyDeviceToHost));
            bool equal = true;
            for (Form f : {F1, F2}) {
                CK(hipMemset(buf, 0x5A, (size_t)CHECK_ROWS * w * 2));
                launch(f, g, sd, d_map + M + 1);
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(got.data(), buf, got.size() * 2, hipMemcpyDeviceToHost));
                equal = equal && !memcmp(got.data(), want.data(), want.size() * 2);
            }
            std::vector<std::vector<float>> t(NFORMS);
            for (int r = 0; r < ROUNDS; ++r)
                for (int f = 0; f < NFORMS; ++f) t[f].push_back(timed((Form)f, g, f == FP32 ? sd32 : sd, d_map + M + 1, ea, eb));
            auto med = [](std::vector<float> v) { std::sort(v.begin(), v.end()); return v[v.size() / 2]; };
            printf("%u | %u |", N, w);
            for (int f = 0; f < NFORMS; ++f) {
                for (float x : t[f]) printf(" %.4f", x);
                printf(" |");
            }
            printf(" %.4f | %.4f | %.4f | %s\n", med(t[PLAIN]) + med(t[PACK]), med(t[F1]), med(t[F2]), equal ? "yes" : "NO");
            fflush(stdout);
            if (!equal) return 2;
        }
        CK(hipFree(B)); CK(hipFree(C)); CK(hipFree(buf));
    }
    CK(hipFree(A)); CK(hipFree(d_map));
    return 0;
}
