// options.cpp -- the one table of the context's keys (csrc/options.hpp): every option with its default, accepted values, model
// and what fixes it; the read-only keys; the action.  dory_create fills dory_ctx::opt from it, dory_set_option validates through
// option_check, dory_configure through option_model_conflict, and -- pure host code -- a test without a GPU reads and asks it
// through dory_option_spec / dory_option_check.
#include <cstdio>
#include <cstring>

#include "../../include/dorylus_host.h"
#include "../csrc/options.hpp"

namespace dory {

#define OPT(ID, name, def, read, ...) {OPT_##ID, name, KIND_OPTION, def, read, ##__VA_ARGS__}
#define RO(ID, name) {OPT_COUNT + RO_##ID, name, KIND_READ_ONLY, 0, READ_CALL}
static constexpr OptionSpec TABLE[] = {
    OPT(SPMM_VARIANT, "spmm_variant", 2, READ_PREALLOC),   // 2: K1s register-accumulating sweep over the blocked adjacency, 1: K1b (partial rows), 0: K1 only
    OPT(SPMM_SWEEP_FLAGS, "spmm_sweep_flags", 0, READ_CALL),   // K1s: reserved for experiments (bit 1 is the library's own "second launch" mark)
    OPT(SPMM_SWEEP_ROWS, "spmm_sweep_rows", 0, READ_LAYOUT),   // K1s: rows per lane group, 0 = by fill (2/4/6/8/10; tests and experiments); the launches read it again
    OPT(SPMM_SWEEP_PAIR, "spmm_sweep_pair", -1, READ_CALL),    // K1s: two rows of a lane group as one stream of entries: -1 = launches of >= 3 slabs, 0 = never, 1 = always
    OPT(SPMM_SWEEP_LOADER, "spmm_sweep_loader", 1, READ_LAYOUT),   // K1s, 32-lane launches: wave 0 of a workgroup copies the next step's entries and offsets into LDS for all sixteen
    OPT(SPMM_SWEEP_LOADER_RELIEF, "spmm_sweep_loader_relief", 3, READ_LAYOUT),   // ... and the layout gives each of its two lane groups this many rows fewer per sweep (set before the layout is built)
    OPT(SPMM_SWEEP_RESERVE_CUS, "spmm_sweep_reserve_cus", 4, READ_CALL),   // K1s under an exchange in flight: CUs per XCD its sweeps leave to the RCCL kernels
    OPT(SPMM_SWEEP_LAYOUT, "spmm_sweep_layout", 3, READ_LAYOUT),   // K1s layout: 1 = spread the source rows over the blocks at random, 2 = deal the rows by degree (0: K1b's order -- graphs without structure only)
    OPT(SPMM_SWEEP_WINDOW_KB, "spmm_sweep_window_kb", 0, READ_LAYOUT),   // K1s: source window per block; 0 = 2432 KB (two live windows in one XCD's 4 MB L2), 3584 KB for partitions of <= 4 rows per lane group
    OPT(SPMM_XCD_ASSUME_MISMATCH, "spmm_xcd_assume_mismatch", 0, READ_CALL),   // testing: treat the placement check as failed (the gated / ungated choice is then made by measurement)
    OPT(SPMM_SLAB, "spmm_slab", 0, READ_CALL),
    OPT(SPMM_ORDER, "spmm_order", 1, READ_UPLOAD),   // K1: rows longest first -- 1 = when the degrees are skewed (max > 8 x mean), 2 = always, 0 = never (0..2: every call);
                                                     // 3 (before dory_graph_upload) = rows by their median source id instead (experiment, profiles/HISTORY.md)
    OPT(SPMM_BLK_GROUP, "spmm_blk_group", 32, READ_LAYOUT),   // K1b: lanes per row (slab = 4*group floats = 512 B)
    OPT(SPMM_BLK_FORCE_SPLIT, "spmm_blk_force_split", 0, READ_CALL),   // testing: always launch local / ghost source blocks separately
    OPT(HALO_OVERLAP, "halo_overlap", 1, READ_CALL),   // let local-source blocks of the next SpMM run under the exchange
    OPT(GAT_LAZY_EDGE_TENSORS, "gat_lazy_edge_tensors", 1, READ_CALL),   // GAT prototype: az / A / dA (one value per destination) are written per edge only when read (download, raw pointer, K1's per-edge path)
    OPT(GAT_REUSE_NSUM, "gat_reuse_nsum", 1, READ_CALL),   // GAT prototype: the backward's dA-weighted aggregation from the forward's neighbour sum (abi_stages.hip)
    OPT(SPMM_EDGE_SPLIT, "spmm_edge_split", 1, READ_UPLOAD),   // K1 on GCN partitions with ghosts: every row's local-source edges first (set before dory_graph_upload)
    // K1s / GAT sweeps: workgroups per sweep and XCD (0 = all CUs of an XCD); its range, 0..CUs per XCD, is the device's: dory_set_option checks it
    OPT(SPMM_SWEEP_CUS, "spmm_sweep_cus", 0, READ_UPLOAD, 1, 0, nullptr, GNN_ANY, ""),
    OPT(LOCAL_TIMEOUT_MS, "local_timeout_ms", 30000, READ_CALL),   // in-process device transport: how long a rank's host thread waits for a peer's host thread
    OPT(ADJACENCY_VALUES_ASYMMETRIC, "adjacency_values_asymmetric", 0, READ_CALL),   // set by dory_partition_upload for undirected / unknown builds: csrVal != cscVal^T
    OPT(GATMH_BWD_PHASE, "gatmh_bwd_phase", 0, READ_CALL),   // multi-head GAT backward: 0 = whole sweep (exchanging the ghost rows itself), 1 / 2 = first / second phase only (callers with their own transport)
    OPT(GATMH_BLOCKED, "gatmh_blocked", 1, READ_PREALLOC),   // multi-head GAT: source-blocked (L2-resident) gathers where the blocked adjacency applies
    OPT(GATMH_EL_ON_THE_FLY, "gatmh_el_on_the_fly", 1, READ_CALL),   // multi-head GAT, blocked forward with fused statistics, heads of <= 16 features: el[src] from the gathered row instead of a second gather
    OPT(GATMH_SWEEP, "gatmh_sweep", 1, READ_PREALLOC),   // multi-head GAT: the edge passes on K1s's skeleton (gat_mh_sweep.hip) where the sweep layout and the shape apply (1: forward)
    OPT(GATMH_SRC_WINDOW_KB, "gatmh_src_window_kb", 0, READ_LAYOUT),   // multi-head GAT: source window of the OUT-edge sweep layout in KB of 512-byte rows (0 = as the forward's, 4608)
    OPT(GATMH_SWEEP_ROWS, "gatmh_sweep_rows", 0, READ_LAYOUT),   // rows per lane group of the multi-head GAT contexts' sweep layouts (0 = by fill, at most 8)
    OPT(GATMH_FUSED_STATS, "gatmh_fused_stats", 1, READ_CALL),   // multi-head GAT, blocked forward: online softmax per source block + merge in the reduce (0: separate statistics pass first)
    OPT(GCN_CACHE_AH0, "gcn_cache_ah0", 0, READ_CALL),   // GCN: keep ah@0 = A_hat x across epochs while x, fg@0 and the adjacency are unchanged (opt-in; the reference recomputes it)
    // GCN: aggregations read their source rows rounded to bf16, fp32 sums: 1 = forward, 2 = forward and backward (opt-in; see dorylus_hip.h)
    OPT(GCN_BF16_GATHER, "gcn_bf16_gather", 0, READ_CALL, 0, 2, "0 (off), 1 (forward) or 2 (forward and backward)", DORY_GCN),
    // GCN, with gcn_bf16_gather: K1s gathers bf16 rows of 128 floats or more eight features per lane (16-byte gathers); same bits (opt-in; see dorylus_hip.h)
    OPT(GCN_BF16_WIDE, "gcn_bf16_wide", 0, READ_CALL, 0, 1, "0 (off) or 1 (16-byte gathers of bf16 rows in K1s)", DORY_GCN),
    // multi-head GAT: the sweep forms' edge passes gather their rows rounded to bf16, fp32 sums: 1 = forward (z), 2 = and the backward's source side (do) (opt-in; see dorylus_hip.h)
    OPT(GATMH_BF16_GATHER, "gatmh_bf16_gather", 0, READ_CALL, 0, 2, "0 (off), 1 (forward) or 2 (forward and the backward's source side)", DORY_GATMH),
    // multi-head GAT, with gatmh_bf16_gather: passes on bf16 rows of 128 floats or more (several heads of 16 / 32 / 64 features) gather eight features per lane (16-byte gathers); same bits (opt-in; see dorylus_hip.h)
    OPT(GATMH_BF16_WIDE, "gatmh_bf16_wide", 0, READ_CALL, 0, 1, "0 (off) or 1 (16-byte gathers of bf16 rows in the multi-head GAT's sweeps)", DORY_GATMH),
    // packed halo rows hold exactly `cols` floats instead of the padded `ld` (every transport and the split entry points; same ghost rows bit for bit; opt-in; see dorylus_hip.h)
    OPT(HALO_EXACT_ROWS, "halo_exact_rows", 0, READ_CALL, 0, 1, "0 (padded rows travel) or 1 (rows of exactly cols floats)"),
    // halo rows land in the ghost tensors themselves, ghost rows stored in wire order: no receive buffer, no unpack (before dory_graph_upload; opt-in; see dorylus_hip.h)
    OPT(HALO_DIRECT_RECV, "halo_direct_recv", 0, READ_UPLOAD, 0, 1, "0 (receive buffer and unpack) or 1 (halo rows land in the ghost tensors, stored in wire order)",
        GNN_ANY, " (the adjacency's ghost numbering depends on it)"),
    OPT(GCN_TRANSFORM_FIRST, "gcn_transform_first", 0, READ_CALL),   // GCN layers as A(XW) instead of (AX)W where the input is wider than the output: 1 = layer 0, 2 = all (see tf_layer)
    OPT(EPOCH_GRAPH, "epoch_graph", 0, READ_ENGINE),   // engine: replay a recorded epoch (hipGraph) when the partition is alone
    OPT(SPMM_BLK_NB, "spmm_blk_nb", 0, READ_LAYOUT),   // K1b: number of source blocks (0 = auto, ~3.75 MB windows); another value rebuilds the layouts
    RO(GCN_CACHE_AH0_SKIPS, "gcn_cache_ah0_skips"),   // layer-0 aggregations answered from the cached ah@0
    RO(GCN_BF16_GATHERS_K1S, "gcn_bf16_gathers_k1s"),             // aggregations on bf16 rows, per kernel family
    RO(GCN_BF16_GATHERS_K1S_WIDE, "gcn_bf16_gathers_k1s_wide"),   // (of _k1s: the wide form, option gcn_bf16_wide)
    RO(GCN_BF16_GATHERS_K1, "gcn_bf16_gathers_k1"),
    // aggregations of spmm() per kernel family that committed to running them (eager calls and recordings, not replays)
    RO(SPMM_LAUNCHES_K1S, "spmm_launches_k1s"), RO(SPMM_LAUNCHES_K1B, "spmm_launches_k1b"), RO(SPMM_LAUNCHES_K1, "spmm_launches_k1"),
    // multi-head GAT edge passes on bf16 rows (_wide: of those, the wide form, option gatmh_bf16_wide)
    RO(GATMH_BF16_GATHERS_FWD, "gatmh_bf16_gathers_fwd"), RO(GATMH_BF16_GATHERS_SRC, "gatmh_bf16_gathers_src"),
    RO(GATMH_BF16_GATHERS_FWD_WIDE, "gatmh_bf16_gathers_fwd_wide"), RO(GATMH_BF16_GATHERS_SRC_WIDE, "gatmh_bf16_gathers_src_wide"),
    // what the eager packs (exchanges and dory_halo_pack*) wrote into send buffers since dory_create, and the packs
    // that ran the exact form of option halo_exact_rows on rows narrower than their padding
    RO(HALO_ROWS_PACKED, "halo_rows_packed"), RO(HALO_FLOATS_PACKED, "halo_floats_packed"), RO(HALO_EXACT_PACKS, "halo_exact_packs"),
    // the exchanges (eager calls and recordings, one step each) whose rows landed in the ghost tensor itself (option
    // halo_direct_recv) / went through the receive buffer and an unpack, and the bytes of that buffer
    RO(HALO_DIRECT_RECVS, "halo_direct_recvs"), RO(HALO_STAGED_RECVS, "halo_staged_recvs"), RO(HALO_RECV_BUF_BYTES, "halo_recv_buf_bytes"),
    RO(EPOCH_GRAPH_RECORDED, "epoch_graph_recorded"),   // does the ctx still hold a recorded epoch?
    RO(SPMM_XCD_MAPPING_OK, "spmm_xcd_mapping_ok"), RO(SPMM_XCD_COUNT, "spmm_xcd_count"),   // dory_create's placement check
    RO(SPMM_XCD_POLICY, "spmm_xcd_policy"),   // -1 undecided / not needed, 0 gated, 8 ungated
    RO(SPMM_XCD_GATED_US, "spmm_xcd_gated_us"), RO(SPMM_XCD_UNGATED_US, "spmm_xcd_ungated_us"),
    // counters of the K1s gates (device words that outlive the launches): timeouts = a sweep's workgroups were not
    // co-resident within the polling bound; ungated launches = launches that ran without gates while the context
    // backed off after a timeout (same results, unsynchronised rate)
    RO(SPMM_GATE_TIMEOUTS, "spmm_gate_timeouts"), RO(SPMM_UNGATED_LAUNCHES, "spmm_ungated_launches"),
    // write: end a K1s gate back-off now (both launch classes), the counters stay; reads as "is a back-off pending"
    {KEY_SPMM_GATES_REARM, "spmm_gates_rearm", KIND_ACTION, 0, READ_CALL},
};
#undef OPT
#undef RO

// the enums and the table cannot drift: a record per key id, each at its own index
constexpr bool table_in_order() {
    for (int i = 0; i < KEY_COUNT; ++i)
        if (TABLE[i].id != i) return false;
    return true;
}
static_assert(sizeof(TABLE) / sizeof(TABLE[0]) == KEY_COUNT, "options: one record per OptionId, ReadOnlyId and the action");
static_assert(table_in_order(), "options: the records are in the order of the enums");

const OptionSpec *option_spec(int id) { return id >= 0 && id < KEY_COUNT ? &TABLE[id] : nullptr; }

int option_find(const char *name) {
    for (int i = 0; name && i < KEY_COUNT; ++i)
        if (!strcmp(name, TABLE[i].name)) return i;
    return -1;
}

static int refuse(char *msg, size_t n, const char *fmt, const char *a, const char *b) {
    if (msg && n) snprintf(msg, n, fmt, a, b);
    return DORY_ERR_ARG;
}

int option_check(int id, int64_t value, int gnn, bool configured, bool has_graph, char *msg, size_t n) {
    const OptionSpec *s = option_spec(id);
    if (!s || s->kind != KIND_OPTION) return refuse(msg, n, "unknown option '%s'%s", s ? s->name : "(null)", "");
    if (s->lo <= s->hi && (value < s->lo || value > s->hi)) return refuse(msg, n, "%s: %s", s->name, s->domain);
    if (s->gnn != GNN_ANY && value && configured && gnn != s->gnn)
        return refuse(msg, n, "%s: %s", s->name, s->gnn == DORY_GCN ? "GCN contexts only" : "multi-head GAT contexts (DORY_GATMH) only");
    if (s->fixed && has_graph) return refuse(msg, n, "%s: set it before the graph is uploaded%s", s->name, s->fixed);
    return DORY_OK;
}

int option_model_conflict(const int64_t *opt, int gnn, char *msg, size_t n) {
    for (int i = 0; i < OPT_COUNT; ++i)
        if (TABLE[i].gnn != GNN_ANY && TABLE[i].gnn != gnn && opt[i])
            return refuse(msg, n, "dory_configure: %s is %s (set it to 0 first)", TABLE[i].name,
                          TABLE[i].gnn == DORY_GCN ? "a GCN option" : "an option of the multi-head GAT");
    return DORY_OK;
}

}  // namespace dory

using namespace dory;

extern "C" {

int dory_option_spec(uint32_t index, const char **name, int *kind, int64_t *def, int64_t *lo, int64_t *hi, int *gnn,
                     int *fixed_by_graph, int *read) {
    const OptionSpec *s = option_spec(index < (uint32_t)KEY_COUNT ? (int)index : -1);
    if (!s) return DORY_ERR_ARG;
    if (name) *name = s->name;
    if (kind) *kind = s->kind;
    if (def) *def = s->def;
    if (lo) *lo = s->lo;
    if (hi) *hi = s->hi;
    if (gnn) *gnn = s->gnn;
    if (fixed_by_graph) *fixed_by_graph = s->fixed != nullptr;
    if (read) *read = s->read;
    return DORY_OK;
}

int dory_option_check(const char *name, int64_t value, int gnn, int configured, int has_graph, char *msg, size_t n) {
    const int id = option_find(name);
    if (id < 0) {
        if (msg && n) snprintf(msg, n, "unknown option '%s'", name ? name : "(null)");
        return DORY_ERR_ARG;
    }
    return option_check(id, value, gnn, configured != 0, has_graph != 0, msg, n);
}

}  // extern "C"
