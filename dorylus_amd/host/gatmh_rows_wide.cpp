// gatmh_rows_wide.cpp -- dory_gatmh_row_gather_bf16_wide_form (include/dorylus_host.h): the shape rule of the row-gather family's wide
// bf16 form as the launchers apply it (csrc/gat_mh_shapes.hpp: gatmh_rows8_form), for tests and tools without a context or a device.
#include "../../include/dorylus_host.h"
#include "../csrc/gat_mh_shapes.hpp"

extern "C" int dory_gatmh_row_gather_bf16_wide_form(uint32_t K, uint32_t D, uint32_t ld, uint32_t *lanes_per_row, uint32_t *lanes_per_head,
                                                    int *scores_from_row) {
    uint32_t lr = 0, lh = 0;
    int el = 0;
    const bool ok = dory::gatmh_rows8_form(K, D, ld, &lr, &lh, &el);
    if (lanes_per_row) *lanes_per_row = ok ? lr : 0;
    if (lanes_per_head) *lanes_per_head = ok ? lh : 0;
    if (scores_from_row) *scores_from_row = ok ? el : 0;
    return ok ? 1 : 0;
}
