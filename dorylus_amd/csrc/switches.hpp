// switches.hpp -- the feature switches of the (ctx, int) shape (dory_halo_fused_pack ... dory_gatmh_row_gather_bf16): their ids, the counters their
// _stats entry points report, and the record host/switches.cpp keeps of each (pure host code: name, highest value, refusals in order, what a successful
// set does before the store, counters).  dory_ctx::sw is indexed by SwitchId, dory_ctx::count by CounterId; the table and the one validator are in
// host/switches.cpp, the one setter path (switch_set) and the hooks of the switches that own memory in csrc/abi_comm.hip.  No HIP in here.
// (dory_gat_bf16_gather(mode, wide) is not in the table: two values, legal before dory_configure, and it reserves buffers.)
#ifndef DORY_SWITCHES_HPP
#define DORY_SWITCHES_HPP
#include <cstddef>
#include <cstdint>

namespace dory {

// the switches, in the order of the table (host/switches.cpp checks at compile time that record i has id i)
enum SwitchId : int {
    SW_HALO_FUSED_PACK, SW_HALO_FUSED_PACK_BF16, SW_HALO_FUSED_PACK_ROWWISE, SW_GATMH_BWD_MERGED_EXCHANGE, SW_GATMH_HALO_BF16,
    SW_HALO_BF16_ROWS, SW_HALO_BF16_GHOSTS, SW_GATMH_BF16_GHOSTS, SW_GATMH_ROW_GATHER, SW_GATMH_ROW_GATHER_BF16,
    SW_COUNT
};
constexpr int SW_NONE = -1;

// what the _stats entry points report (dorylus_hip.h says what each counts), a line per switch in the order of the table
enum CounterId : int {
    CNT_FUSED_EXCHANGES, CNT_FUSED_ROWS, CNT_FALLBACK_EXCHANGES, CNT_FUSED_BF16_EXCHANGES, CNT_FUSED_BF16_ROWS, CNT_ROWWISE_EXCHANGES, CNT_ROWWISE_ROWS,
    CNT_MERGED_EXCHANGES, CNT_MERGED_ROWS, CNT_MERGED_PRODUCER_PACKED, CNT_MERGED_SPLIT_FALLBACKS,
    CNT_GATMH_FWD_BF16_EXCHANGES, CNT_GATMH_BWD_BF16_EXCHANGES, CNT_GATMH_BWD_BF16_ROWS, CNT_GATMH_PRODUCER_PACKED_BF16,
    CNT_HALO_BF16_PACKS, CNT_HALO_BF16_BYTES, CNT_HALO_FP32_PACKS_WHILE_ON,
    CNT_GHOST_LANDED_DIRECT, CNT_GHOST_LANDED_BY_KERNEL, CNT_GHOST_CONVERSIONS_SKIPPED, CNT_GHOST_WIDENED,
    CNT_GATMH_TWIN_FWD, CNT_GATMH_TWIN_BWD, CNT_GATMH_TWIN_BWD_MERGED, CNT_GATMH_TWIN_READS_ROWS, CNT_GATMH_TWIN_READS_SWEEP,
    CNT_GATMH_TWIN_SCORES, CNT_GATMH_TWIN_WIDENED,
    CNT_GATMH_ROWS_FWD, CNT_GATMH_ROWS_DST_EDGE, CNT_GATMH_ROWS_DST_ROWWISE, CNT_GATMH_ROWS_SRC,
    CNT_GATMH_ROWS_BF16_FWD, CNT_GATMH_ROWS_BF16_DST_EDGE, CNT_GATMH_ROWS_BF16_SRC,
    CNT_COUNT
};

// what a setter asks of the context before it takes a value: a refusal names a set of them and fires when any one fails
enum SwitchCond : unsigned {
    COND_VALUE = 1u,               // 0 <= value <= SwitchSpec::hi
    COND_CONFIGURED = 2u,          // dory_configure has run
    COND_GATMH = 4u,               // the model is DORY_GATMH
    COND_GATMH_IF_NONZERO = 8u,    // a nonzero value needs a context configured as DORY_GATMH ("off" is legal on any)
    COND_PREALLOC = 16u,           // dory_preallocate has run
    COND_NOT_RECORDING = 32u,      // no epoch graph is being recorded
    COND_PARENT_ON = 64u           // the switch this one lives on top of (SwitchSpec::parent) is on
};
struct SwitchRefusal { unsigned conds = 0 /* 0: the end of the list */; const char *text = nullptr /* after "<name>: " */; };
constexpr int SW_MAX_REFUSALS = 5, SW_MAX_COUNTERS = 7;

struct SwitchSpec {
    int id;                        // its index in the table
    const char *name;              // its entry point is dory_<name>, its counters' dory_<name>_stats
    int hi, parent;                // accepted values 0..hi; SW_NONE, or the switch COND_PARENT_ON asks for
    bool waits_halo, drops_stamp;  // a successful set first waits for the halo in flight / drops the fused pack's stamp
    SwitchRefusal refusals[SW_MAX_REFUSALS];   // in the order the setter checks them
    int ncounters, counters[SW_MAX_COUNTERS];  // CounterIds in the order of the _stats signature
    bool twin_bytes = false;       // _stats has one more, computed entry behind them: the bytes of all bf16 twins
};

const SwitchSpec *switch_spec(int id);   // 0 <= id < SW_COUNT, else null
// would dory_<name>(ctx, value) take `value` on a context of this state?  DORY_OK, or DORY_ERR_ARG and in msg "<name>: <text>" of the first refusal that fires
int switch_check(int id, int value, int gnn, bool configured, bool prealloc, bool recording, bool parent_on, char *msg, size_t n);

}  // namespace dory
#endif
