// halo_bf16_keep_forms.hip -- the two lane forms of scatter_rows_bf16_keep_kernel (csrc/elementwise.hip: copies of it) side by side:
// eight elements per lane (two 8-byte loads of the stream, one 16-byte store into the twin) against four (one 8-byte load, one
// 8-byte store), at the shapes of tools/halo_bf16_rate.py -- 3.15 M rows, identity slots, 10 launches after a warm one, 3 rounds
// alternating.  The faster form is the one the library instantiates (profiles/HISTORY.md section 21 has the numbers).
//   hipcc --offload-arch=gfx950 -O3 -std=c++17 tools/probes/halo_bf16_keep_forms.hip -o tools/probes/halo_bf16_keep_forms
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
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

template <int LE>
__global__ __launch_bounds__(256) void keep_kernel(uint16_t *dst, const uint2 *src, uint32_t ld, uint32_t re4, const uint32_t *rows, uint32_t n) {
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

template <int LE>
static float run(uint16_t *dst, const uint2 *src, uint32_t ld, uint32_t re, const uint32_t *rows, uint32_t n, hipEvent_t a, hipEvent_t b) {
    const uint64_t total = (uint64_t)n * (ld / LE);
    const int blocks = (int)((total + 255) / 256 < 2048 ? (total + 255) / 256 : 2048);
    for (int i = 0; i < 11; ++i) {
        if (i == 1) CK(hipEventRecord(a, nullptr));
        hipLaunchKernelGGL(keep_kernel<LE>, dim3(blocks), dim3(256), 0, nullptr, dst, src, ld, re / 4, rows, n);
    }
    CK(hipEventRecord(b, nullptr));
    CK(hipEventSynchronize(b));
    float ms = 0.f;
    CK(hipEventElapsedTime(&ms, a, b));
    return ms / 10.f;
}

int main(int argc, char **argv) {
    const uint32_t n = argc > 1 ? (uint32_t)atoll(argv[1]) : 3u << 20;
    const struct { uint32_t cols, re, ld; } shapes[] = {{64, 64, 64}, {300, 320, 320}, {300, 300, 320}, {128, 128, 128},
                                                       {48, 64, 64},  {48, 48, 64},    {41, 64, 64},    {41, 44, 64}};
    std::vector<uint32_t> ident(n);
    std::iota(ident.begin(), ident.end(), 0u);
    uint32_t *rows = nullptr;
    CK(hipMalloc((void **)&rows, (size_t)n * 4));
    CK(hipMemcpy(rows, ident.data(), (size_t)n * 4, hipMemcpyHostToDevice));
    hipEvent_t a, b;
    CK(hipEventCreate(&a));
    CK(hipEventCreate(&b));
    printf("# %u rows; ms per launch (mean of 10 after a warm one), 3 rounds alternating 8 / 4 elements per lane\n", n);
    printf("# cols row_elems ld | keep8 (rounds) | keep4 (rounds)\n");
    for (const auto &s : shapes) {
        uint16_t *dst = nullptr;
        uint2 *src = nullptr;
        CK(hipMalloc((void **)&dst, (size_t)n * s.ld * 2));
        CK(hipMalloc((void **)&src, (size_t)n * s.re * 2));
        CK(hipMemset(src, 0x3c, (size_t)n * s.re * 2));
        float t8[3], t4[3];
        for (int r = 0; r < 3; ++r) {
            t8[r] = run<8>(dst, src, s.ld, s.re, rows, n, a, b);
            t4[r] = run<4>(dst, src, s.ld, s.re, rows, n, a, b);
        }
        printf("%u %u %u | %.4f %.4f %.4f | %.4f %.4f %.4f |\n", s.cols, s.re, s.ld, t8[0], t8[1], t8[2], t4[0], t4[1], t4[2]);
        fflush(stdout);
        CK(hipFree(dst));
        CK(hipFree(src));
    }
    CK(hipFree(rows));
    return 0;
}
