// k1_fp8.cpp -- dory_k1_fp8_rows and dory_k1_fp8_form (include/dorylus_hip.h): the number format of K1's fp8 row gather as a plain
// host function (what fp8_rows_kernel, csrc/spmm_fp8.hip, must give byte for byte) and the form rule as launch_k1_fp8 applies it
// (csrc/k1_shapes.hpp: k1_fp8_form), for tests and tools without a context or a device.
#include <cmath>
#include <cstring>

#include "../../include/dorylus_hip.h"
#include "../csrc/k1_shapes.hpp"

namespace {

// |y| <= 448 -> OCP E4M3 (float8_e4m3fn), round to nearest even, subnormals (steps of 2^-9 below 2^-6) included; the sign is kept
uint8_t e4m3_rne(float y) {
    const uint8_t sign = std::signbit(y) ? 0x80 : 0;
    const float a = std::fabs(y);
    if (!(a > 0.f)) return sign;
    int ex = -6;
    if (a >= 0.015625f) { (void)std::frexp(a, &ex); ex -= 1; }        // floor(log2 a)
    const float step = std::ldexp(1.f, (a >= 0.015625f ? ex : -6) - 3);
    const float n = a / step;                                             // exact: a power of two divides
    float r = std::floor(n);
    const float d = n - r;
    if (d > 0.5f || (d == 0.5f && std::fmod(r, 2.f) == 1.f)) r += 1.f;
    const float v = r * step;
    if (v < 0.015625f) return sign | (uint8_t)r;                          // subnormal: r in 0 .. 7
    int e2;
    const float f = std::frexp(v, &e2);                                   // v = f 2^e2, f in [0.5, 1): the rounding may have reached the next binade
    return sign | (uint8_t)(((e2 - 1 + 7) << 3) | (int)((f * 2.f - 1.f) * 8.f));
}

}  // namespace

extern "C" int dory_k1_fp8_rows(const float *rows, uint64_t n, uint32_t cols, uint32_t ld, uint8_t *q_out, uint8_t *e_out) {
    if (ld < cols || (n && cols && !rows) || (n && ld && !q_out) || (n && !e_out)) return DORY_ERR_ARG;
    for (uint64_t i = 0; i < n; ++i) {
        const float *x = rows + i * cols;
        float amax = 0.f;
        for (uint32_t j = 0; j < cols; ++j) amax = std::fmax(amax, std::fabs(x[j]));
        int e = 0;
        if (amax > 0.f) {
            int k;
            (void)std::frexp(amax, &k);                                   // amax = f 2^k, f in [0.5, 1): floor(log2 amax) = k - 1
            e = k - 1 - 7;
            e = e < DORY_K1_FP8_EXP_MIN ? DORY_K1_FP8_EXP_MIN : (e > DORY_K1_FP8_EXP_MAX ? DORY_K1_FP8_EXP_MAX : e);
        }
        e_out[i] = (uint8_t)(e + 127);
        uint8_t *q = q_out + i * ld;
        for (uint32_t j = 0; j < cols; ++j) {
            float y = std::ldexp(x[j], -e);
            y = y > 448.f ? 448.f : (y < -448.f ? -448.f : y);
            q[j] = e4m3_rne(y);
        }
        if (ld > cols) std::memset(q + cols, 0, ld - cols);
    }
    return DORY_OK;
}

extern "C" int dory_k1_fp8_form(uint32_t ld, uint32_t slab, uint32_t *lanes, uint32_t *chunks, uint32_t *bytes_per_lane) {
    uint32_t g = 0, k = 0, b = 0;
    const bool ok = dory::k1_fp8_form(ld, slab, &g, &k, &b);
    if (lanes) *lanes = ok ? g : 0;
    if (chunks) *chunks = ok ? k : 0;
    if (bytes_per_lane) *bytes_per_lane = ok ? b : 0;
    return ok ? 1 : 0;
}
