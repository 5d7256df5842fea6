// k1_rows_wide.cpp -- dory_k1_bf16_wide_form (include/dorylus_hip.h): the form rule of K1's wide bf16 row gather as launch_spmm
// applies it (csrc/k1_shapes.hpp: k1_rows8_form), for tests and tools without a context or a device.
#include "../../include/dorylus_hip.h"
#include "../csrc/k1_shapes.hpp"

extern "C" int dory_k1_bf16_wide_form(uint32_t ld, uint32_t slab, uint32_t *lanes, uint32_t *chunks) {
    uint32_t g = 0, k = 0;
    const bool ok = dory::k1_rows8_form(ld, slab, &g, &k);
    if (lanes) *lanes = ok ? g : 0;
    if (chunks) *chunks = ok ? k : 0;
    return ok ? 1 : 0;
}
