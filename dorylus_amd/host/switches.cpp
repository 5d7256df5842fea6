// switches.cpp -- the one table of the feature switches (csrc/switches.hpp): every switch with its highest value, its refusals in the order its
// setter checks them, what a successful set does before the store, and the counters of its _stats entry point.  switch_set (csrc/abi_comm.hip)
// validates through switch_check, and -- pure host code -- a test without a GPU reads and asks the table through dory_switch_spec / dory_switch_check.
#include <cstdio>
#include <cstring>

#include "../../include/dorylus_host.h"
#include "../csrc/switches.hpp"

namespace dory {

static constexpr const char *RECORDING = "not while an epoch graph is being recorded";
static constexpr const char *CONFIGURE_FIRST = "dory_configure first; on is 0 or 1";
static constexpr const char *GATMH_CONFIGURED = "a context configured as DORY_GATMH; on is 0 or 1";

static constexpr const char *GHOSTS_FIRST = "dory_configure and dory_preallocate first (the twins of the tensors are allocated here); on is 0 or 1";

// {id, name, hi, parent, waits for the halo, drops the stamp,
//  {refusals},
//  counters, {counters}}
static constexpr SwitchSpec TABLE[] = {
    {SW_HALO_FUSED_PACK, "halo_fused_pack", 1, SW_NONE, true, true,   // (legal inside a recording: the recorded exchanges never fuse)
     {{COND_CONFIGURED | COND_VALUE, CONFIGURE_FIRST}},
     3, {CNT_FUSED_EXCHANGES, CNT_FUSED_ROWS, CNT_FALLBACK_EXCHANGES}},
    {SW_HALO_FUSED_PACK_BF16, "halo_fused_pack_bf16", 1, SW_NONE, true, true,
     {{COND_CONFIGURED | COND_VALUE, CONFIGURE_FIRST}, {COND_NOT_RECORDING, RECORDING}},
     2, {CNT_FUSED_BF16_EXCHANGES, CNT_FUSED_BF16_ROWS}},
    {SW_HALO_FUSED_PACK_ROWWISE, "halo_fused_pack_rowwise", 1, SW_NONE, true, true,
     {{COND_CONFIGURED | COND_VALUE, CONFIGURE_FIRST}, {COND_NOT_RECORDING, RECORDING}},
     2, {CNT_ROWWISE_EXCHANGES, CNT_ROWWISE_ROWS}},
    {SW_GATMH_BWD_MERGED_EXCHANGE, "gatmh_bwd_merged_exchange", 1, SW_NONE, true, false,   // (no stamp names do or st)
     {{COND_CONFIGURED | COND_GATMH | COND_VALUE, GATMH_CONFIGURED}, {COND_NOT_RECORDING, RECORDING}},
     4, {CNT_MERGED_EXCHANGES, CNT_MERGED_ROWS, CNT_MERGED_PRODUCER_PACKED, CNT_MERGED_SPLIT_FALLBACKS}},
    {SW_GATMH_HALO_BF16, "gatmh_halo_bf16", 1, SW_NONE, true, true,
     {{COND_CONFIGURED | COND_GATMH | COND_VALUE, GATMH_CONFIGURED}, {COND_NOT_RECORDING, RECORDING}},
     4, {CNT_GATMH_FWD_BF16_EXCHANGES, CNT_GATMH_BWD_BF16_EXCHANGES, CNT_GATMH_BWD_BF16_ROWS, CNT_GATMH_PRODUCER_PACKED_BF16}},
    {SW_HALO_BF16_ROWS, "halo_bf16_rows", 1, SW_NONE, true, true,
     {{COND_CONFIGURED | COND_VALUE, CONFIGURE_FIRST}, {COND_NOT_RECORDING, RECORDING}},
     3, {CNT_HALO_BF16_PACKS, CNT_HALO_BF16_BYTES, CNT_HALO_FP32_PACKS_WHILE_ON}},
    {SW_HALO_BF16_GHOSTS, "halo_bf16_ghosts", 1, SW_NONE, true, true,
     {{COND_CONFIGURED | COND_PREALLOC | COND_VALUE, GHOSTS_FIRST}, {COND_NOT_RECORDING, RECORDING}},
     4, {CNT_GHOST_LANDED_DIRECT, CNT_GHOST_LANDED_BY_KERNEL, CNT_GHOST_CONVERSIONS_SKIPPED, CNT_GHOST_WIDENED}, true},
    {SW_GATMH_BF16_GHOSTS, "gatmh_bf16_ghosts", 1, SW_HALO_BF16_GHOSTS, true, true,
     {{COND_CONFIGURED | COND_GATMH, "a context configured as DORY_GATMH"},
      {COND_PREALLOC, "dory_preallocate first (the twins of fg_z and bg_do are allocated here)"},
      {COND_VALUE, "on is 0 or 1"},
      {COND_NOT_RECORDING, RECORDING},
      {COND_PARENT_ON, "dory_halo_bf16_ghosts is off (turn it on first: this switch lives on top of it)"}},
     7, {CNT_GATMH_TWIN_FWD, CNT_GATMH_TWIN_BWD, CNT_GATMH_TWIN_BWD_MERGED, CNT_GATMH_TWIN_READS_ROWS, CNT_GATMH_TWIN_READS_SWEEP,
         CNT_GATMH_TWIN_SCORES, CNT_GATMH_TWIN_WIDENED}},
    // the row-gather pair: read by the next aggregation only -- no exchange in flight and no stamp depends on them
    {SW_GATMH_ROW_GATHER, "gatmh_row_gather", 1, SW_NONE, false, false,
     {{COND_VALUE, "mode is 0 or 1"},
      {COND_GATMH_IF_NONZERO, "mode 1 needs a context configured as DORY_GATMH"},
      {COND_NOT_RECORDING, RECORDING}},
     4, {CNT_GATMH_ROWS_FWD, CNT_GATMH_ROWS_DST_EDGE, CNT_GATMH_ROWS_DST_ROWWISE, CNT_GATMH_ROWS_SRC}},
    {SW_GATMH_ROW_GATHER_BF16, "gatmh_row_gather_bf16", 1, SW_NONE, false, false,
     {{COND_VALUE, "on is 0 or 1"},
      {COND_GATMH_IF_NONZERO, "on = 1 needs a context configured as DORY_GATMH"},
      {COND_NOT_RECORDING, RECORDING}},
     3, {CNT_GATMH_ROWS_BF16_FWD, CNT_GATMH_ROWS_BF16_DST_EDGE, CNT_GATMH_ROWS_BF16_SRC}},
};

// the enum and the table cannot drift: a record per switch id, each at its own index
constexpr bool table_in_order() {
    for (int i = 0; i < SW_COUNT; ++i)
        if (TABLE[i].id != i) return false;
    return true;
}
static_assert(sizeof(TABLE) / sizeof(TABLE[0]) == SW_COUNT, "switches: one record per SwitchId");
static_assert(table_in_order(), "switches: the records are in the order of the enum");

const SwitchSpec *switch_spec(int id) { return id >= 0 && id < SW_COUNT ? &TABLE[id] : nullptr; }

int switch_check(int id, int value, int gnn, bool configured, bool prealloc, bool recording, bool parent_on, char *msg, size_t n) {
    const SwitchSpec *s = switch_spec(id);
    if (!s) return DORY_ERR_ARG;
    const bool gatmh = gnn == DORY_GATMH;
    const unsigned failed = (value < 0 || value > s->hi ? COND_VALUE : 0u) | (configured ? 0u : COND_CONFIGURED) | (gatmh ? 0u : COND_GATMH) |
                            (value != 0 && !(configured && gatmh) ? COND_GATMH_IF_NONZERO : 0u) | (prealloc ? 0u : COND_PREALLOC) |
                            (recording ? COND_NOT_RECORDING : 0u) | (parent_on ? 0u : COND_PARENT_ON);
    for (const SwitchRefusal &r : s->refusals)
        if (r.conds & failed) {
            if (msg && n) snprintf(msg, n, "%s: %s", s->name, r.text);
            return DORY_ERR_ARG;
        }
    if (msg && n) msg[0] = 0;
    return DORY_OK;
}

}  // namespace dory

using namespace dory;

extern "C" {

int dory_switch_spec(uint32_t index, const char **name, int *hi, int *refusals, int *waits_halo, int *drops_stamp, int *parent, int *counters) {
    const SwitchSpec *s = switch_spec(index < (uint32_t)SW_COUNT ? (int)index : -1);
    if (!s) return DORY_ERR_ARG;
    if (name) *name = s->name;
    if (hi) *hi = s->hi;
    if (refusals) *refusals = 0;
    for (const SwitchRefusal &r : s->refusals) if (refusals && r.conds) ++*refusals;
    if (waits_halo) *waits_halo = s->waits_halo;
    if (drops_stamp) *drops_stamp = s->drops_stamp;
    if (parent) *parent = s->parent;
    if (counters) *counters = s->ncounters + s->twin_bytes;
    return DORY_OK;
}

int dory_switch_check(const char *name, int value, int gnn, int configured, int prealloc, int recording, int parent_on, char *msg, size_t n) {
    for (int id = 0; name && id < SW_COUNT; ++id)
        if (!strcmp(name, TABLE[id].name)) return switch_check(id, value, gnn, configured != 0, prealloc != 0, recording != 0, parent_on != 0, msg, n);
    if (msg && n) snprintf(msg, n, "unknown switch '%s'", name ? name : "(null)");
    return DORY_ERR_ARG;
}

}  // extern "C"
