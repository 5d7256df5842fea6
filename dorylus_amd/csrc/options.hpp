// options.hpp -- the keys of dory_set_option / dory_get_option: their ids, and the record host/options.cpp keeps of each (pure
// host code: default, accepted values, model, what fixes it, when it is read).  dory_ctx::opt is indexed by OptionId; the
// table, option_find and the one validator are in host/options.cpp.  No HIP in here.
#ifndef DORY_OPTIONS_HPP
#define DORY_OPTIONS_HPP
#include <cstddef>
#include <cstdint>

namespace dory {

// the options, in the order of the table (host/options.cpp checks at compile time that record i has id i)
enum OptionId : int {
    OPT_SPMM_VARIANT, OPT_SPMM_SWEEP_FLAGS, OPT_SPMM_SWEEP_ROWS, OPT_SPMM_SWEEP_PAIR, OPT_SPMM_SWEEP_LOADER, OPT_SPMM_SWEEP_LOADER_RELIEF,
    OPT_SPMM_SWEEP_RESERVE_CUS, OPT_SPMM_SWEEP_LAYOUT, OPT_SPMM_SWEEP_WINDOW_KB, OPT_SPMM_XCD_ASSUME_MISMATCH, OPT_SPMM_SLAB, OPT_SPMM_ORDER,
    OPT_SPMM_BLK_GROUP, OPT_SPMM_BLK_FORCE_SPLIT, OPT_HALO_OVERLAP, OPT_GAT_LAZY_EDGE_TENSORS, OPT_GAT_REUSE_NSUM, OPT_SPMM_EDGE_SPLIT,
    OPT_SPMM_SWEEP_CUS, OPT_LOCAL_TIMEOUT_MS, OPT_ADJACENCY_VALUES_ASYMMETRIC, OPT_GATMH_BWD_PHASE, OPT_GATMH_BLOCKED, OPT_GATMH_EL_ON_THE_FLY,
    OPT_GATMH_SWEEP, OPT_GATMH_SRC_WINDOW_KB, OPT_GATMH_SWEEP_ROWS, OPT_GATMH_FUSED_STATS, OPT_GCN_CACHE_AH0, OPT_GCN_BF16_GATHER,
    OPT_GCN_BF16_WIDE, OPT_GATMH_BF16_GATHER, OPT_GATMH_BF16_WIDE, OPT_HALO_EXACT_ROWS, OPT_HALO_DIRECT_RECV, OPT_GCN_TRANSFORM_FIRST,
    OPT_EPOCH_GRAPH, OPT_SPMM_BLK_NB,
    OPT_COUNT
};
// the read-only keys of dory_get_option: key id OPT_COUNT + ReadOnlyId (a type of its own: the switch that answers them
// has no default, so the compiler names a key it misses)
enum ReadOnlyId : int {
    RO_GCN_CACHE_AH0_SKIPS, RO_GCN_BF16_GATHERS_K1S, RO_GCN_BF16_GATHERS_K1S_WIDE, RO_GCN_BF16_GATHERS_K1,
    RO_SPMM_LAUNCHES_K1S, RO_SPMM_LAUNCHES_K1B, RO_SPMM_LAUNCHES_K1,
    RO_GATMH_BF16_GATHERS_FWD, RO_GATMH_BF16_GATHERS_SRC, RO_GATMH_BF16_GATHERS_FWD_WIDE, RO_GATMH_BF16_GATHERS_SRC_WIDE,
    RO_HALO_ROWS_PACKED, RO_HALO_FLOATS_PACKED, RO_HALO_EXACT_PACKS, RO_HALO_DIRECT_RECVS, RO_HALO_STAGED_RECVS, RO_HALO_RECV_BUF_BYTES,
    RO_EPOCH_GRAPH_RECORDED,
    RO_SPMM_XCD_MAPPING_OK, RO_SPMM_XCD_COUNT, RO_SPMM_XCD_POLICY, RO_SPMM_XCD_GATED_US, RO_SPMM_XCD_UNGATED_US,
    RO_SPMM_GATE_TIMEOUTS, RO_SPMM_UNGATED_LAUNCHES,
    RO_COUNT
};
// ... and the one action: a set rearms the K1s gates, a get reads "is a back-off pending"
constexpr int KEY_SPMM_GATES_REARM = OPT_COUNT + RO_COUNT;
constexpr int KEY_COUNT = KEY_SPMM_GATES_REARM + 1;

enum OptionKind : int { KIND_OPTION = 0, KIND_READ_ONLY = 1, KIND_ACTION = 2 };
// When the library reads an option -- the earliest of its reads, after which a new value no longer reaches everything built
// from the old one.  Documentation: only OptionSpec::fixed is enforced.
enum OptionRead : int {
    READ_CALL = 0,      // by every call that it concerns
    READ_UPLOAD = 1,    // by dory_graph_upload (or, spmm_sweep_cus, at the set itself for what the upload builds)
    READ_PREALLOC = 2,  // by dory_preallocate, which builds the layouts the calls then find; the calls read it again
    READ_LAYOUT = 3,    // when a blocked / sweep layout is built: dory_preallocate, or the first aggregation that needs one
    READ_ENGINE = 4     // by dory_engine_run, not by the library's stages
};
constexpr int GNN_ANY = -1;

struct OptionSpec {
    int id;                        // its index in the table
    const char *name;
    OptionKind kind;
    int64_t def;                   // options: the value dory_create gives it
    OptionRead read;
    int64_t lo = 1, hi = 0;        // accepted values lo..hi; lo > hi: any int64_t
    const char *domain = nullptr;  // ranged options: the text of the refusal, after "<name>: "
    int gnn = GNN_ANY;             // the model (dory_gnn) a nonzero value needs
    const char *fixed = nullptr;   // non-null: refused once a graph is uploaded; the reason that follows the refusal's text
};

const OptionSpec *option_spec(int id);   // 0 <= id < KEY_COUNT, else null
int option_find(const char *name);       // key id, or -1 (null and unknown names)
// Would dory_set_option take `value` for option id on a context of this state?  DORY_OK, or DORY_ERR_ARG with the refusal in
// msg: its range first, then its model (a nonzero value on a configured context of another model), then the uploaded graph.
// (spmm_sweep_cus's upper bound is the device's: dory_set_option checks it afterwards.)
int option_check(int id, int64_t value, int gnn, bool configured, bool has_graph, char *msg, size_t n);
// dory_configure(gnn): the first nonzero option that belongs to another model -- DORY_ERR_ARG and the refusal, or DORY_OK
int option_model_conflict(const int64_t *opt, int gnn, char *msg, size_t n);

}  // namespace dory
#endif
