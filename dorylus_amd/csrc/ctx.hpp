// ctx.hpp -- internal state behind the C-ABI (include/dorylus_hip.h).
// MI355X / gfx950 only; no CUDA shims, no dual paths.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/dorylus_hip.h"
#include "options.hpp"
#include "switches.hpp"
#include "sweep_geometry.hpp"
#include "row_chunks.hpp"
#include "k1_shapes.hpp"

namespace dory {

// Device tensor: row-major fp32, leading dimension padded to 32 floats (one
// 128-B line) so that every row starts on a cache-line boundary and float4
// lanes never straddle rows (602 -> 608).  Host layout stays dense.
struct Tensor {
    uint64_t rows = 0;
    uint32_t cols = 0;
    uint32_t ld = 0;
    float *d = nullptr;
    bool owned = true;  // false: alias of another allocation (GAT "A" = csc values)
    bool raw_handed = false;   // dory_tensor_info has handed out its device pointer: never the target of a fused halo pack again
    // dory_halo_bf16_ghosts: the bf16 twin of a ghost tensor -- rows x ld bf16 in the tensor's own row order, allocated by the
    // setter / dory_preallocate, freed with the tensor (free_table) -- and which of the two copies holds the current rows
    // (DORY_GHOST_FP32 / _TWIN / _BOTH).  null: no twin (every other tensor; one-column ghost tensors): always DORY_GHOST_FP32.
    uint16_t *twin = nullptr;
    int twin_state = DORY_GHOST_FP32;
    size_t bytes() const { return (size_t)rows * ld * sizeof(float); }
    size_t twin_bytes() const { return (size_t)rows * ld * sizeof(uint16_t); }
    bool twin_current() const { return twin && twin_state != DORY_GHOST_FP32; }
};

inline uint32_t pad_ld(uint32_t cols) { return cols <= 1 ? cols : (cols + 31u) & ~31u; }

struct Timing {
    double total_ms = 0;
    uint64_t launches = 0;
};

struct HaloPlan {
    bool set = false;
    std::vector<uint32_t> send_counts, recv_counts;  // per peer (rows)
    std::vector<uint32_t> send_off, recv_off;        // prefix sums
    uint32_t send_total = 0, recv_total = 0;
    uint32_t *d_send_lvids = nullptr;  // concat over peers
    uint32_t *d_recv_slots = nullptr;  // concat over peers
    // option halo_direct_recv (the value when the plan was made): received row r is stored at ghost row r, and recv_slots[r]
    // (`order`, on the device d_recv_slots) is the caller-visible ghost index of that row -- what dory_tensor_upload / download /
    // fill_uniform of a ghost tensor permute by.  d_unpack_slots is what the unpack kernels scatter by: d_recv_slots, or under
    // the option an identity list of its own (a staged exchange and dory_halo_unpack* copy row r to ghost row r).
    bool direct = false;
    std::vector<uint32_t> order;
    uint32_t *d_unpack_slots = nullptr;
    // the fused halo pack (dory_halo_fused_pack): the send list turned round, row -> slots of the packed send buffer, as
    // dory_halo_send_map makes it -- one allocation of row_ptr[N + 1] followed by row_slots[send_total]; null: not built
    uint32_t *d_send_map = nullptr;
    uint32_t send_map_rows = 0;   // the N it was built for (a graph uploaded again with another N: no fusing until the next plan)
};
// The fused halo pack's stamp: the rows of `src` lie in `buf` (the context's send buffer as it was then) packed for the exchange
// of direction `dir` at w floats per row, written by a GEMM epilogue.  abi_comm.hip makes, matches and drops it.
struct FusedStamp {
    const Tensor *src = nullptr;   // null: no stamp
    int dir = 0;
    uint32_t w = 0;
    const float *buf = nullptr;
    bool bf16 = false;   // dory_halo_fused_pack_bf16: the rows are bf16 (w elements of 2 bytes, the first `cols` hold values)
    uint32_t cols = 0;
    bool rowwise = false;   // dory_halo_fused_pack_rowwise: who wrote them -- a row-wise producer's send form, not a GEMM epilogue
};

// The wire format of a packed halo row: w elements per row -- the tensor's padded ld, or with `exact` (option halo_exact_rows)
// its cols -- of 4 bytes (fp32), or with `bf16` (dory_halo_bf16_rows) of 2: then w is rounded up to a multiple of 4 elements and
// `cols` of them hold values, the rest zeros.  Made by row_wire() (abi_comm.hip) alone; which pack / unpack kernels run and the
// zeroing of [w, ld) follow from it, and every byte count of an exchange from row_bytes().
// dory_gatmh_bwd_merged_exchange: w2 != 0 makes it a merged row [w floats of the first tensor | w2 floats of a second] (fp32, both
// multiples of 4: a row starts on a 16-byte boundary) -- the pair kernels pack and unpack it.
struct RowWire {
    uint32_t w = 0;
    bool exact = false;
    bool bf16 = false;
    uint32_t cols = 0;   // (bf16 only: the columns of the tensor below w that the pack reads)
    uint32_t w2 = 0;     // (merged rows only: the floats of the second tensor behind the first's w)
    // dory_gatmh_halo_bf16: a merged row whose first part is bf16 -- [w bf16 of the first tensor | w2 fp32 of the second], w a multiple of
    // 8 (the second part starts on a 16-byte boundary, the row is w / 2 + w2 floats, a multiple of 4); `bf16` with w2 != 0 means that
    uint32_t elem_bytes() const { return bf16 ? 2u : 4u; }
    size_t row_bytes() const { return w2 ? ((size_t)(bf16 ? w / 2 : w) + w2) * 4u : (size_t)w * elem_bytes(); }
};
// The second tensor of an exchange of merged rows (the multi-head GAT's st -> bg_st behind do -> bg_do), and whether the producer has
// written the send rows into the context's send buffer already (gatmh_dst_rowwise_send_kernel): then the exchange runs no pack.
struct RowPair {
    const Tensor *src2 = nullptr;
    Tensor *ghost2 = nullptr;
    bool producer_packed = false;
};

// Scatter messages (dory_scatter_msgs_*, abi_comm.hip): the id tables of dory_halo_wire_ids, the round stamps and counters of
// the unpack, the fixed staging area of dory_scatter_msgs_deliver, the message tables of the layouts asked for so far, and the
// scatter transport's callback with its send buffers.
struct ScatterLayout {
    int dir = 0;
    uint32_t cols = 0, max_rows = 0;
    uint64_t max_msg = 0, total_bytes = 0;
    std::vector<dory_scatter_msg> msgs;
    dory_scatter_msg *d_msgs = nullptr;
};
struct ScatterState {
    bool ids = false;
    uint32_t *d_l2g = nullptr;                      // N
    std::vector<uint32_t> gvids[2];                 // per direction: the ghosts' global ids, ascending (slot order)
    uint32_t *d_gvids[2] = {nullptr, nullptr};
    uint32_t *d_slot_row[2] = {nullptr, nullptr};   // option halo_direct_recv: ghost slot -> stored (wire-order) row; null: identity
    uint32_t *d_stamp[2] = {nullptr, nullptr};      // per ghost slot: the round that wrote it last
    uint32_t *d_counts[2] = {nullptr, nullptr};     // rows written, unknown ids, duplicates of the round in progress
    uint32_t round[2] = {1, 1};
    std::vector<ScatterLayout> layouts;
    // staging: slot i is free again when ev_stage[i] has happened (the unpack that read it)
    uint8_t *h_stage[2] = {nullptr, nullptr};
    uint8_t *d_stage[2] = {nullptr, nullptr};
    hipEvent_t ev_stage[2] = {nullptr, nullptr};
    bool stage_used[2] = {false, false};
    size_t stage_bytes = 0;
    int next_slot = 0;
    // transport
    dory_scatter_exchange_fn fn = nullptr;
    uint64_t max_msg = 0;
    uint8_t *d_send = nullptr, *h_send = nullptr;
    size_t send_cap = 0;
    // the exchange whose callback is running (on cb_thread): its ghost tensor, and what the headers must say
    std::atomic<bool> in_cb{false};
    std::thread::id cb_thread;
    Tensor *cb_ghost = nullptr;
    uint32_t cb_layer = 0;
    int cb_dir = 0;
};

// K1b: source-blocked adjacency (per-block CSR over the virtual source space [local;ghost])
struct BlockedAdj {
    uint32_t nb = 0;        // number of source blocks (multiple of 8: one per XCD per round)
    uint32_t SB = 0;        // rows per block
    uint32_t row_bytes = 0; // slab bytes per row the block size was chosen for
    uint32_t npos = 0;      // destination positions = leading dimension of boff minus 1 (N, or more with `perm`)
    uint32_t nb_local = 0;  // blocks [0, nb_local) contain local source rows only
    uint32_t nghost = 0;    // K1s layout: ghost source rows (blocks [nb_local, nb) contain only those)
    uint32_t rows_per_group = 0;   // K1s layout: the R its positions were dealt for
    // K1s layout (build_blocked_sweep): destination positions are a degree-balanced deal of the rows (rows of very high
    // degree cut into pieces), source rows are spread over the blocks by a random permutation (local / ghost rows apart)
    uint32_t *perm = nullptr;        // npos: position -> row, 0xFFFFFFFF = empty; nullptr = identity
    uint32_t *otgt = nullptr;        // npos: where a position's sum goes: the row, or 0x80000000 | slot for a piece of a split row
    uint32_t *split_rows = nullptr;  // 3 words per split row: row, first slot, pieces
    uint32_t nsplit = 0, nslots = 0;
    uint64_t *bbase = nullptr;  // nb+1: first edge of each block
    uint32_t *boff = nullptr;   // [nb][N+1]: row offsets inside the block
    uint32_t *bidx = nullptr;   // nnz: source row (virtual id), block-major / row-minor / edge order
    float *bval = nullptr;      // nnz
    uint2 *bent = nullptr;      // K1s layout: (bidx, bval bits) interleaved instead of the two arrays (nnz + 2 entries, 16-byte aligned pairs)
    // (block,row) segments longer than BLK_SEG_CLAMP edges (hubs): K1b stops there, the remainder is cut into chunks
    // of BLK_SEG_CHUNK edges for workgroup-per-chunk kernels (spmm.hip); all empty on graphs without such segments
    uint32_t seg_clamp = 0;             // 0: no long segments
    uint32_t nsegs = 0, nchunks = 0;
    uint32_t *seg_row = nullptr;        // nsegs: destination row
    uint32_t *seg_blk = nullptr;        // nsegs: source block
    uint32_t *seg_chunk_ptr = nullptr;  // nsegs+1
    uint32_t *seg_chunks = nullptr;     // 6 words per chunk: row, block, e0 (lo, hi), e1 (lo, hi): absolute positions in bidx
};
constexpr uint32_t BLK_SEG_CLAMP = 2048, BLK_SEG_CHUNK = 4096;
// K1's long rows (hubs): the part of a row beyond LONG_ROW_CLAMP edges, in chunks of LONG_ROW_CHUNK edges
constexpr uint32_t LONG_ROW_CLAMP = 8192, LONG_ROW_CHUNK = 4096;
// (LongRowsHost, the output of plan_long_rows: row_chunks.hpp -- 6 words per chunk = struct LongChunk)
// K1 beside an exchange in flight (round 6): every row's edges regrouped local sources first, ghost sources after (stable), so
// that ONE pass over all rows sums the local part while the ghost rows are still travelling and a second pass adds the rest --
// the row gather's counterpart of K1s's local-source blocks.  The interior / boundary ROW split it replaces hides nothing on
// a graph where nearly every row has a ghost neighbour (mean degree 25, 15 % remote edges: 98 % of the rows).
struct EdgeSplit {
    uint32_t *idx = nullptr;   // nnz: source ids, local ones first within every row
    float *val = nullptr;      // nnz
    uint64_t *mid = nullptr;   // N: first ghost-source edge of the row
};
// the row-gather family of the multi-head GAT beside an exchange in flight (dory_gatmh_row_gather_edge_split): the same regrouping
// (row_chunks.hpp: plan_row_edge_split) and the rows that have a ghost entry at all -- the units of the launch after the wait
struct RowsEdgeSplit {
    uint32_t *idx = nullptr;    // nnz: ids, local ones first within every row (stable)
    uint64_t *mid = nullptr;    // N: the row's first ghost entry (ptr[v + 1]: none)
    uint32_t *brows = nullptr;  // nbrows: the rows with mid[v] < ptr[v + 1], ascending
    uint32_t nbrows = 0;
    uint64_t local = 0;         // entries with a local id
    bool built = false;
};
struct LongRowsDev {
    uint32_t nrows = 0, nchunks = 0;
    uint32_t *rows = nullptr, *row_chunk_ptr = nullptr, *chunks = nullptr;
};
// a layout derived from one adjacency (built on first use) with its state
struct DerivedAdj : BlockedAdj {
    bool built = false;
    bool na = false;        // not applicable to this graph: the next kernel family takes the aggregation
    uint32_t want_nb = 0;   // the spmm_blk_nb it was built for
};
// One direction of the graph (Graph, graph/graph.hpp:60-99) and everything built from it.  dory_ctx::adj[ADJ_IN] is the CSC of
// the in-edges = the reference's forwardAdj (ptr: column pointers, idx: source rows, ghosts: ghost sources); adj[ADJ_OUT] is the
// CSR of the out-edges = backwardAdj (row pointers, destination columns, ghost destinations).
struct Adjacency {
    uint64_t *ptr = nullptr;   // N+1
    uint32_t *idx = nullptr;   // nnz, local ids; >= N means ghost row idx-N
    float *val = nullptr;      // nnz
    uint64_t nnz = 0;
    uint32_t ghosts = 0;
    // longest-row-first schedule for the SpMM (built at upload)
    uint32_t *order = nullptr;
    bool skew = false;           // max degree > 8 x mean: K1 walks the rows longest first (option spmm_order = 1)
    // K1 under a halo exchange in flight: rows whose sources are all local ("interior", first n_interior entries) run
    // first, the rows that read ghost rows after the exchange; both parts longest row first
    uint32_t *split = nullptr;   // N entries: interior rows, then boundary rows
    uint32_t n_interior = 0;
    LongRowsDev long_rows;       // K1: hub rows
    // dory_gatmh_row_gather_hub_split: the rows with more than hub_chunk entries, whole, in chunks of hub_chunk entries (the row-gather
    // family of the multi-head GAT; built by hub_plan_ensure when the value is set or at first use, dropped with the adjacency)
    LongRowsDev hub_rows;
    uint32_t hub_chunk = 0;      // the chunk size hub_rows was planned for (0: no plan)
    // dory_gatmh_row_gather_overlap: the rows in launch order (N entries) -- first the rows_first rows a launch beside an exchange may hold,
    // ascending: the interior rows of plan_row_interior (every entry < N) that the hub plan of rows_hub_chunk does not cut; then all other
    // rows, ascending.  Built by interior_plan_ensure when the switch is set or at first use, dropped with the adjacency
    uint32_t *rows_split = nullptr;
    uint32_t rows_first = 0, rows_interior = 0;   // (rows_interior: the plan's interior rows, cut or not)
    uint32_t rows_hub_chunk = 0;
    bool rows_split_built = false;
    EdgeSplit edge_split;        // K1: local-first copy (GCN partitions with ghosts)
    // dory_gatmh_row_gather_edge_split: the row-gather family's own local-first copy (no per-edge values: only ids move) -- built from
    // the ids as uploaded by rows_edge_ensure when the switch is set or at first use, dropped with the adjacency
    RowsEdgeSplit rows_edge;
    DerivedAdj blk;              // K1b blocked copy; na: too many source blocks, use K1
    // multi-head GAT contexts with layers on both sides of 128 floats: a second copy, blocked for the 256-B slabs of the narrow
    // layers (K1b's windows hold a fixed number of BYTES: 24 blocks of 512-B rows, 16 of 256-B rows at Reddit size)
    DerivedAdj blk16;
    DerivedAdj swp;              // K1s layout (when spmm_variant == 2)
};
enum { ADJ_IN = 0, ADJ_OUT = 1 };
// In-process device transport (dory_comm_init_local, abi_comm.hip): the contexts of one process that are each other's
// peers.  Peers read each other's plans, buffers, events and progress counters; nothing else.
struct LocalGroup {
    std::mutex mu;                    // membership only (a context leaving at dory_destroy)
    std::vector<dory_ctx *> ctx;      // by rank; nullptr once destroyed
};
struct AdamState {
    float lr = 0.01f;
    unsigned epochs = 1;  // AdamOptimizer ctor calls nextIteration() once
    float lr_t = 0.f;
};

}  // namespace dory

struct dory_ctx {
    int device = 0;
    std::mutex mu;
    std::string err;
    hipStream_t compute = nullptr, comm = nullptr;
    bool own_compute = false, own_comm = false;
    hipEvent_t ev_a = nullptr, ev_b = nullptr;  // cross-stream ordering
    bool halo_pending = false;  // ghosts of the last exchange are still landing (comm stream, ev_b)

    // model
    bool configured = false;
    int gnn = DORY_GCN;
    uint32_t L = 0;
    std::vector<uint32_t> dims;
    uint32_t globalV = 0, nodeId = 0, numNodes = 1;
    std::vector<uint32_t> heads;   // multi-head GAT extension: heads per layer

    // graph (Graph, graph/graph.hpp:60-99)
    bool has_graph = false;
    uint32_t N = 0;
    float *norm = nullptr;
    dory::Adjacency adj[2];                     // [ADJ_IN] forwardAdj, [ADJ_OUT] backwardAdj
    bool agg_static_ghosts = false;             // the aggregation being issued reads ghost rows no exchange writes (layer 0 forward)
    uint32_t cus_per_xcd = 32;                  // K1s: workgroups per sweep
    // K1s's placement assumption, checked once per context (dory_create: HW_REG_XCC_ID of 2048 probe workgroups -- equal
    // id & 7 => same XCD, the eight residues on eight XCDs).  When it does not hold (a CPX / NPS-partitioned or CU-masked device) the gates
    // synchronise workgroups that do not share an L2: the first idempotent K1s launch is then run gated and ungated, timed,
    // and the faster form kept (xcd_policy: -1 not decided, 0 gated, 8 ungated = the SWEEP flag)
    bool xcd_mapping_ok = true;
    uint32_t xcd_count = 8;
    int xcd_policy = -1;
    float xcd_gated_ms = 0.f, xcd_ungated_ms = 0.f;
    uint32_t *sweep_stat = nullptr;             // K1s: SWEEP_STAT_WORDS device words that outlive the launches: gate timeouts, back-off horizon of
                                                // the launches that run alone, ungated launches, back-off horizon of the launches
                                                // beside an exchange, launch number (bumped on the device: hipGraph replays advance
                                                // it), workgroups of the launch in flight that have left
    // GAT: per-destination edge factors written by dory_apply_edge are valid for these layers
    std::vector<char> gat_arow_valid, gat_drow_valid;
    // GAT prototype, "gat_lazy_edge_tensors": the per-edge tensors az / A / dA hold one value per DESTINATION; the stages keep the
    // per-vertex values (azrow / arow / drow) and write the per-edge copies only when somebody asks for them
    std::vector<char> gat_azrow_valid;              // azrow@l describes az@l (false after a caller uploaded az)
    std::vector<char> gat_az_stale, gat_dA_stale;   // per layer: az@l / dA@l are behind azrow@l / drow@l
    int gat_A_stale_layer = -1;                     // "A" (= forwardAdj.values) is behind arow@this layer
    std::vector<char> gat_nsum_valid;    // GAT prototype: "nsum"@l holds the unweighted neighbour sum of the current z / fg_z (forward -> backward)
    std::vector<char> gat_nsum_bf16;     // ... summed over rows rounded to bf16 (dory_gat_bf16_gather was on when the forward made it)
    bool gat_ones_set = false;           // "ones"@0 filled
    bool last_spmm_unit = false;         // the last spmm() gathered with unit weights and a per-row factor (K1s / K1b), not with per-edge values (K1)
    std::vector<char> gatmh_fwd_swept;   // multi-head GAT: the forward of this layer left "op" / "dpos" (the sweep skeleton, or the row-gather family)
    // dory_gatmh_row_gather_bf16, per layer: this layer's forward ran the row-gather family's bf16 form (its m / den are statistics
    // of rounded rows: the destination-side edge pass has to gather the same)
    std::vector<char> gatmh_fwd_rows_bf16;
    // dory_gatmh_row_gather_hub_split: entries per chunk (0 = off), and the forward / destination-side edge / source-side passes that ran split
    uint32_t gatmh_hub_chunk = 0;
    uint64_t gatmh_hub_fwd = 0, gatmh_hub_dst = 0, gatmh_hub_src = 0;
    // dory_gatmh_row_gather_overlap: the switch; forward / source-side passes that ran as interior rows + the rest, those of them with an
    // exchange in flight beside the interior launch, and the backward exchanges issued deferred for it
    bool gatmh_rows_overlap = false;
    int gatmh_scores_pending = -1;   // the layer whose ghost sources' scores (fg_el / fg_er) wait for the exchange in flight; -1: none
    uint64_t gatmh_ovl_fwd = 0, gatmh_ovl_src = 0, gatmh_ovl_fwd_flight = 0, gatmh_ovl_src_flight = 0, gatmh_ovl_deferred = 0;
    // dory_gatmh_row_gather_edge_split: the value (0 off, 1 two launches around an exchange in flight and one otherwise, 2 always two);
    // forward / source-side passes that ran the carry kernels, those of them with an exchange in flight beside the first launch, passes
    // left to the hub chunk plan, bf16 passes that ran the narrow carry kernel with dory_gatmh_row_gather_bf16_wide on; and the states
    // of the rows between the two launches -- a buffer of its own (nothing between the launches may write it: wait_halo's deferred score
    // kernels, the ghost rows' conversion, an unpack and launch_gatmh_dattn all use other memory), grown outside a recording only
    int gatmh_edge_split = 0;
    uint64_t gatmh_es_fwd = 0, gatmh_es_src = 0, gatmh_es_fwd_flight = 0, gatmh_es_src_flight = 0, gatmh_es_hub_fallbacks = 0,
             gatmh_es_wide_not_taken = 0;
    float *gatmh_carry_state = nullptr;
    size_t gatmh_carry_bytes = 0;
    // dory_gatmh_row_gather_bf16_wide: the switch; the forward / destination-side edge / source-side passes that ran the wide bf16 form, and
    // the bf16 passes of the family that ran narrow with the switch on (shape or alignment)
    bool gatmh_rows_wide = false;
    uint64_t gatmh_rows8_fwd = 0, gatmh_rows8_dst = 0, gatmh_rows8_src = 0, gatmh_rows8_narrow = 0;
    // dory_k1_bf16_wide: the switch; the aggregations on bf16 rows that K1 ran in its wide form, and those it ran narrow with the switch
    // on (no form for the row or slab width, rows not 16-byte aligned)
    bool k1_bf16_wide = false;
    uint64_t k1_rows8_wide = 0, k1_rows8_narrow = 0;
    float *partial = nullptr;
    size_t partial_bytes = 0;

    // tensors / weights
    bool prealloc = false;
    bool ah0_valid = false;      // option gcn_cache_ah0: ah@0 holds the aggregate of the current x / fg@0 / adjacency
    uint64_t ah0_skips = 0;      // layer-0 aggregations answered from it
    // options gcn_bf16_gather / gatmh_bf16_gather: the bf16 copy of the rows an aggregation reads ((N + ghosts) x ld, rewritten
    // by every pass that uses it, never kept across calls), and the passes that ran on it per kernel family
    uint16_t *bf16_rows = nullptr;
    size_t bf16_rows_bytes = 0;
    uint64_t bf16_gathers_k1s = 0, bf16_gathers_k1 = 0, bf16_gathers_k1s_wide = 0;   // (_wide: those of _k1s that ran the wide form, option gcn_bf16_wide)
    // dory_gat_bf16_gather (GAT prototype): mode 0 / 1 / 2, the wide form of K1s, and the aggregations that ran on bf16 rows per
    // kernel family (_wide: those of _k1s that ran the wide form; fallbacks: requested on bf16 rows, run on fp32 rows)
    int gat_bf16_mode = 0;
    bool gat_bf16_wide = false;
    uint64_t gat_bf16_gathers_k1s = 0, gat_bf16_gathers_k1s_wide = 0, gat_bf16_gathers_k1 = 0, gat_bf16_fp32_fallbacks = 0;
    uint64_t spmm_launches_k1s = 0, spmm_launches_k1b = 0, spmm_launches_k1 = 0;   // aggregations per kernel family (read-only options of the same names)
    uint64_t gatmh_bf16_gathers_fwd = 0, gatmh_bf16_gathers_src = 0;   // multi-head GAT: forward edge passes, source-side passes
    uint64_t gatmh_bf16_gathers_fwd_wide = 0, gatmh_bf16_gathers_src_wide = 0;   // (those of them that ran the wide form, option gatmh_bf16_wide)
    std::vector<std::map<std::string, dory::Tensor>> tensors;   // [layer][name]
    std::vector<std::map<std::string, dory::Tensor>> weights;   // "w", "a_i"
    std::vector<std::map<std::string, dory::Tensor>> wgrads;    // same names
    std::vector<std::map<std::string, dory::Tensor>> adam_m, adam_v;
    dory::AdamState adam;

    // scratch
    float *scratch = nullptr;
    size_t scratch_bytes = 0;
    float *d_stat = nullptr;  // [acc_sum, loss_sum]
    float *d_stat3 = nullptr; // dory_train_stat_global: [acc_sum, loss_sum, validation rows] of this partition, then of all
    uint32_t val_rows = 0;

    // halo
    dory::HaloPlan plan[2];
    float *send_buf = nullptr, *recv_buf = nullptr;
    size_t send_cap = 0, recv_cap = 0;
    // option halo_exact_rows (a copy the peers of the local transport may read without this context's lock), and what the
    // eager packs wrote into send buffers since dory_create: rows, floats, packs that ran the exact form with cols < ld
    std::atomic<int> halo_exact{0};
    uint64_t halo_rows_packed = 0, halo_floats_packed = 0, halo_exact_packs = 0;
    // option halo_direct_recv (a copy the peers of the local transport may read without this context's lock; fixed once a graph
    // is uploaded: the adjacency's ghost numbering depends on it), and the exchanges (eager calls and recordings) whose rows
    // landed in the ghost tensor itself / went through a receive buffer and an unpack
    std::atomic<int> halo_direct{0};
    uint64_t halo_direct_recvs = 0, halo_staged_recvs = 0;
    // The feature switches (switches.hpp; all default 0) by SwitchId, read through sw_on / sw_value below -- atomics: the peers of the local
    // transport read each other's without this context's lock -- the counters of their _stats entry points by CounterId, the fused pack's one stamp
    std::atomic<int> sw[dory::SW_COUNT] = {};
    uint64_t count[dory::CNT_COUNT] = {};
    dory::FusedStamp fused_stamp;
    // the gather modes the rule of dory_halo_bf16_rows reads (options gcn_bf16_gather / gatmh_bf16_gather, dory_gat_bf16_gather's mode); peers read them likewise
    std::atomic<int> gcn_bf16_mode{0}, gat_bf16_mode_pub{0}, gatmh_bf16_mode_pub{0};
    dory::ScatterState scatter;  // scatter messages (dory_scatter_msgs_*) and the scatter transport
    void *nccl = nullptr;  // ncclComm_t
    // host transport (dory_comm_set_host_transport): callbacks + host staging
    dory_alltoallv_fn tx_a2a = nullptr;
    dory_allreduce_fn tx_ar = nullptr;
    void *tx_user = nullptr;
    std::vector<float> tx_send, tx_recv;
    int rank = 0, nranks = 1;
    // in-process device transport (dory_comm_init_local): rows travel device -> device on the sender's comm stream, ordered
    // by cross-context events; a context only ever waits (on the device) for events its peer has ALREADY recorded -- the
    // host side checks the peer's progress counter first -- so no stream depends on a host call still to come
    std::shared_ptr<dory::LocalGroup> local;
    hipEvent_t ev_sent[2] = {nullptr, nullptr};    // [seq & 1]: my rows of exchange seq have landed in the peers' receive buffers
    hipEvent_t ev_cons[2] = {nullptr, nullptr};    // [seq & 1]: my receive buffer of exchange seq has been unpacked (halo_direct_recv: I have copied my rows of exchange seq out of the peers' send buffers)
    hipEvent_t ev_gready[2] = {nullptr, nullptr};  // [seq & 1]: my weight gradient of sum seq is final
    hipEvent_t ev_gdone[2] = {nullptr, nullptr};   // [seq & 1]: I have read every peer's gradient of sum seq
    std::atomic<uint64_t> posted_sent{0}, posted_cons{0}, posted_g{0}, posted_gdone{0};   // last seq whose event is recorded
    uint64_t local_seq = 0, local_ar_seq = 0;      // exchanges / gradient sums issued so far
    struct LocalPending {                           // second half of a deferred exchange (wait for the peers' rows, unpack)
        bool on = false;
        int dir = 0;
        char *ghost = nullptr;                      // where the rows land: the ghost tensor's fp32 rows, or (keep) its bf16 twin
        uint32_t ghost_ld = 0;
        float *ghost2 = nullptr;                    // merged rows (RowWire::w2): the second ghost tensor and its ld
        uint32_t ghost2_ld = 0;
        dory::RowWire wire;                         // what the rows in recv_buf look like (exact: the unpack zeroes [w, ghost_ld))
        bool direct = false;                        // halo_direct_recv and w == ghost_ld: the peers' segments are copied into the ghost tensor (or twin) itself
        bool keep = false;                          // dory_halo_bf16_ghosts: bf16 rows stay bf16, in the twin
        float *widen_to = nullptr;                  // ... and are widened into these fp32 rows at once (the tensor's raw pointer is out)
        uint64_t ghost_rows = 0;
        hipEvent_t t_halo_b = nullptr, t_kind_b = nullptr;   // timing: end events of the "halo" / "halo_deferred|waited" intervals
    } local_pending;
    std::vector<char> local_sent_to;  // halo_direct_recv: the peers that read my send buffer in the last exchange (they pull; I pack again after their "consumed")
    float *ar_tmp = nullptr;          // gradient sum before it replaces the local gradient
    size_t ar_tmp_cap = 0;

    // epoch graph (hipGraph replay of one captured epoch; single partition)
    bool capturing = false;
    hipGraph_t epoch_graph = nullptr;
    hipGraphExec_t epoch_exec = nullptr;
    float *d_lr_table = nullptr;       // Adam step size of each replay of the current launch batch
    uint32_t lr_table_cap = 0;
    uint32_t lr_table_left = 0;        // prepared entries not yet consumed by a replay
    uint32_t *d_replay_idx = nullptr;  // bumped by the last node of the graph
    std::vector<float> lr_table_host;

    // options / timing
    int64_t opt[dory::OPT_COUNT] = {};   // by dory::OptionId; dory_create fills it from the table (host/options.cpp)
    bool timing = false;
    std::map<std::string, dory::Timing> times;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
    struct Pending { std::string fam; hipEvent_t a, b; };
    std::vector<Pending> pending;
};

namespace dory {

// the one way to read a feature switch: its value (dory_gatmh_row_gather's mode), or "is it on"
inline int sw_value(const dory_ctx *c, SwitchId id) { return c->sw[id].load(std::memory_order_acquire); }
inline bool sw_on(const dory_ctx *c, SwitchId id) { return sw_value(c, id) == 1; }

// ---- kernel launchers (one translation unit per family) ---------------------
// K1  CSR/CSC SpMM with fused self term:
//   out[v,:] = self[v]*xl[v,:] + sum_e val[e] * row(idx[e])   (self = norm | 1 | none)
struct SpmmArgs {
    uint32_t N;             // rows (local vertices)
    uint32_t F;             // logical feature width
    uint32_t ld;            // leading dimension of xl, xg, out (all equal)
    const uint64_t *ptr;    // N+1
    const uint32_t *idx;    // nnz, local ids; >= N means ghost row idx-N
    const float *val;       // nnz
    const float *self_scale;// N or nullptr
    int self_mode;          // 0: no self term, 1: self_scale[v]*xl[v], 2: 1*xl[v]
    const float *xl;        // N x ld
    const float *xg;        // G x ld (may be nullptr when no ghosts)
    float *out;             // N x ld
    int accumulate;         // 1: out += result (GAT backward second pass)
    uint32_t row_clamp;     // K1: edges of a row beyond this many are left to the long-row kernels (0 = no limit)
    uint32_t rows;          // K1: rows of this launch = the first `rows` entries of `order` (0 = all N rows)
    const uint32_t *order;  // optional row schedule (longest first) or nullptr
    const uint64_t *ptr_end;// K1: end of every row's edge range (nullptr: ptr[v + 1]); with accumulate == 2 the sum STARTS from out[v]
};
// bf16: xl / xg point at bf16 rows of ld elements (launch_bf16_rows; option gcn_bf16_gather), the sums stay fp32; wide: those rows
// gathered 16 bytes a lane (dory_k1_bf16_wide) -- a form of k1_rows8_form (k1_shapes.hpp) and 16-byte aligned rows, else refused
hipError_t launch_spmm(const SpmmArgs &a, int slab, hipStream_t s, bool bf16 = false, bool wide = false);

void plan_long_rows(const uint64_t *ptr, uint32_t N, LongRowsHost *out);
hipError_t launch_spmm_long_rows(const SpmmArgs &a, const LongRowsDev &L, float *partial /*nchunks x ld*/, hipStream_t s, bool bf16 = false);

hipError_t build_blocked(const uint64_t *ptr, const uint32_t *idx, const float *val, uint32_t N, uint32_t NG,
                         uint64_t nnz, uint32_t want_nb /*0 = auto*/, uint32_t row_bytes, BlockedAdj *out,
                         hipStream_t s, uint64_t window_bytes = 0 /*0 = K1b's windows*/);
uint32_t plan_blocks(uint32_t NG, uint32_t want_nb, uint32_t row_bytes, uint64_t window_bytes = 0);
hipError_t launch_spmm_blocked_part(const SpmmArgs &a, const BlockedAdj &B, float *partial, int group, bool unit,
                                    uint32_t b_lo, uint32_t b_hi, hipStream_t s);
// the long (block,row) segments' remainder added into their partial rows (between the part launches and the reduce)
hipError_t launch_spmm_blocked_long_segments(const SpmmArgs &a, const BlockedAdj &B, float *partial, bool unit,
                                             float *chunk_partial /*nchunks x ld*/, hipStream_t s);
hipError_t launch_spmm_blocked_reduce(const SpmmArgs &a, const BlockedAdj &B, const float *partial,
                                      const float *row_scale, hipStream_t s);
void free_blocked(BlockedAdj *B);
// K1s: the register-accumulating sweep over its own even layout of the blocked adjacency (spmm.hip)
hipError_t build_blocked_sweep(const uint64_t *ptr, const uint32_t *idx, const float *val, uint32_t N, uint32_t NG,
                               uint64_t nnz, uint32_t want_nb, uint32_t row_bytes, uint64_t window_bytes, int R,
                               BlockedAdj *out, hipStream_t s, uint32_t layout = 3 /* 1: spread sources, 2: deal rows by degree */,
                               uint32_t sweep_tiles = 32 /* workgroups per sweep and XCD the deal is made for */,
                               uint32_t loader_relief = 0 /* rows per sweep kept off the two lane groups of every workgroup's wave 0 */);
// host/sweep_deal.cpp: rows per lane group of the K1s layout and the position of every (sorted) item
bool sweep_deal_plan(uint32_t nl, uint32_t R, uint32_t sweep_tiles, std::vector<uint32_t> *cap, uint32_t *npos, uint32_t loader_relief = 0);
bool sweep_deal_positions(uint32_t nl, uint32_t R, const std::vector<uint32_t> &cap, uint32_t *pos, uint32_t loader_lo = 0);
bool sweep_deal_balanced(uint32_t nl, uint32_t R, const std::vector<uint32_t> &cap, const uint64_t *w, uint32_t *pos);
// host/sweep_geometry.cpp: the rows per lane group of a launch on the sweep skeleton, and the geometry that follows from them
int sweep_pick_r(uint32_t N, int group, uint32_t G, int force_r = 0 /* option spmm_sweep_rows: 0 = by fill */, int max_r = 10);
// K1s's row rule: the rows a launch on `group` lanes walks on a layout dealt for rows_per_group (the wide form: ask for 16 lanes)
int sweep_rows(uint32_t rows_per_group, uint32_t npos, int group, uint32_t G, int force_r /* option spmm_sweep_rows */);
bool sweep_wide_rows_ok(int R);   // K1s's wide form has kernels for R rows per 16-lane group
SweepGeometry sweep_geometry(uint32_t npos, uint32_t ld, int group, int R, bool wide, uint32_t G);
size_t sweep_counter_bytes(const SweepGeometry &g, uint32_t nblocks);   // what a launch over nblocks source blocks clears
// ... and the bound callers size the counters by: any launch of that shape, whatever it leaves to concurrent kernels
size_t sweep_counter_bound(uint32_t npos, uint32_t ld, int group, int R, bool wide, uint32_t G, uint32_t nblocks);
bool sweep_supported(const SpmmArgs &a, const BlockedAdj &B, int group);
// per-context knobs and state of the K1s launches (nothing process-wide)
struct SweepCtl {
    int pair = -1;              // option spmm_sweep_pair
    bool loader = true;         // option spmm_sweep_loader: wave 0 of a workgroup copies the next step's entries for all (32-lane launches)
    uint32_t *stat = nullptr;   // SWEEP_STAT_WORDS device words that outlive the launches (dory_ctx::sweep_stat)
};
constexpr int SWEEP_STAT_WORDS = 8;
// One launch on the sweep skeleton over the blocks [b_lo, b_hi) of a sweep layout: what K1s's launcher and those of the multi-head
// GAT's edge passes take alike (abi_stages.hip: SweepLaunch hands them out; sweep_core.hpp: sweep_plan turns one into a launch)
struct SweepPart {
    uint32_t cus;            // workgroups per sweep and XCD
    uint32_t b_lo, b_hi;     // the blocks of the sweep layout this launch walks
    bool accumulate;         // the second launch of an aggregation: go on from the sums the first left (the ghost blocks of a partitioned run)
    uint32_t reserve;        // CUs per XCD left to concurrent kernels (an exchange in flight)
    int R;                   // rows per lane group: the actual count (sweep_rows, gatmh_sweep_rows), one that has a kernel
    uint32_t *done;          // gate counters: sweep_counter_bytes() of device memory
    SweepCtl ctl;
    uint32_t flags;          // SweepArgs::flags but 2 and 32, which follow from accumulate and reserve
    hipStream_t s;
    bool bf16;               // the rows gathered are bf16 rows of ld elements (launch_bf16_rows; options gcn_bf16_gather, gatmh_bf16_gather)
    bool wide;               // bf16 rows, eight features per lane on 16-lane groups (options gcn_bf16_wide, gatmh_bf16_wide)
};
// K1s's wide form (spmm_sweep_bf16x8_kernel): rows of 128 floats or more, 16-lane groups on 128-feature slabs whatever `group`,
// R16 = sweep_rows(.., 16, ..) rows
inline bool sweep_wide_applies(uint32_t ld, int group, int R16) { return ld >= 128 && (group == 16 || group == 32) && sweep_wide_rows_ok(R16); }
// out (+)= self + (row_scale *) sum over the source blocks of p (row_scale: unit edge weights; on bf16 rows the GAT prototype's
// forms, dory_gat_bf16_gather); split_partial: B.nslots x ld floats
hipError_t launch_spmm_sweep(SpmmArgs a, const BlockedAdj &B, int group, const float *row_scale, float *split_partial, const SweepPart &p);
hipError_t launch_spmm_sweep_combine(const SpmmArgs &a, const BlockedAdj &B, const float *row_scale, const float *split_partial,
                                     hipStream_t s, bool bf16 = false);
// fp32 -> bf16 (round to nearest even) of n elements, n a multiple of 4: the rows an aggregation reads under options
// gcn_bf16_gather / gatmh_bf16_gather (elementwise.hip)
hipError_t launch_bf16_rows(const float *x, uint16_t *y, uint64_t n, hipStream_t s);
hipError_t launch_occupy_cus(uint32_t workgroups, uint64_t usec, hipStream_t s);   // diagnostic (dory_debug_occupy_cus)
hipError_t launch_xcd_probe(uint32_t *xcc /*grid words*/, uint32_t grid, hipStream_t s);   // HW_REG_XCC_ID of every probe workgroup
size_t blocked_partial_bytes(const SpmmArgs &a, const BlockedAdj &B);
hipError_t launch_spmm_blocked(const SpmmArgs &a, const BlockedAdj &B, float *partial, int group /*8|16|32 lanes per row*/,
                               const float *row_scale /*nullable: unit edge weights, per-row factor*/, hipStream_t s);

// K2  fp32 MFMA GEMM  C = op(A) op(B) with fused epilogues
enum GemmEpilogue { EPI_NONE = 0, EPI_TANH = 1 /* also writes tanh(C) to C2 */ };
struct GemmArgs {
    int ta, tb;             // op(A): M x K, op(B): K x N
    uint32_t M, N, K;
    const float *A; uint32_t lda;
    const float *B; uint32_t ldb;
    float *C; uint32_t ldc;
    float *C2; uint32_t ldc2;   // EPI_TANH: h = tanh(z)
    int epilogue;
    // prologue on A (NN / TN only): A'[i,k] = A[i,k] * (1 - tanh(Zp[i,k])^2)
    const float *Zp; uint32_t ldz;
};
hipError_t launch_gemm(const GemmArgs &g, float *scratch, size_t scratch_bytes, hipStream_t s);
// The fused halo pack (dory_halo_fused_pack): the extra argument of K2's send kernels.  Row r of the product is also stored at the
// rows row_slots[row_ptr[r] .. row_ptr[r + 1]) of buf, w floats each -- w == the tensor's ld (a padded wire row: [cols, w) gets
// zeros) or == cols (halo_exact_rows: dense rows); `which`: 0 the rows of C, 1 those of the tanh output C2.
// bf16 (dory_halo_fused_pack_bf16; the send16 kernels): buf is addressed in 2-byte elements, a row is w of them (a multiple of 4; w <=
// ld), rounded with pack_bf16x2, zeros in [cols, w) -- what gather_rows_bf16_kernel leaves.
struct GemmSend {
    float *buf;
    const uint32_t *row_ptr;     // M + 1 (dory_halo_send_map)
    const uint32_t *row_slots;   // row_ptr[M]
    uint32_t w, which, cols;
    uint32_t bf16;               // the element kind: 0 fp32, 1 bf16
};
// NN and NT with M, K > 0: *fused = true and the rows are in buf; anything else runs as launch_gemm and leaves *fused false
hipError_t launch_gemm_send(const GemmArgs &g, const GemmSend &sd, float *scratch, size_t scratch_bytes, hipStream_t s, bool *fused);
size_t gemm_scratch_bytes(uint32_t M, uint32_t N, uint32_t K);

// tanh of the transform's epilogue (K2), of the stand-alone activation and of K3's backward -- one function for all three, so
// that h and the 1 - tanh^2 of the backward pass are the same number.  libm's tanhf is ~40 vector instructions (40 M of the
// 53.6 M of a 602->128 launch, round 4); this one is 13: an odd polynomial below 0.35 (Taylor through x^11: the next term is
// 1.2e-8 relative there) and 1 - 2 / (1 + exp(2x)) above (v_exp_f32 + v_rcp_f32; at most ~3e-7 relative at the crossover,
// where the subtraction costs most).  tests/test_gpu_parity.py::test_tanh_matches_libm: <= 1e-6 relative against the oracle.
__device__ __forceinline__ float dory_tanh(float x) {
#ifdef DORY_TANH_LIBM
    return tanhf(x);
#endif
    const float ax = fabsf(x), x2 = x * x;
    float p = fmaf(x2, 0.0088632355f, -0.021869488f);          // 1382/155925, -62/2835
    p = fmaf(x2, p, 0.053968254f);                              // 17/315
    p = fmaf(x2, p, -0.13333333f);                              // -2/15 ... signs alternate: tanh x = x - x^3/3 + 2x^5/15 - 17x^7/315 + 62x^9/2835 - 1382x^11/155925
    p = fmaf(x2, p, 0.33333334f);
    const float small = fmaf(-x * x2, p, x);                    // x - x^3 (1/3 - x^2 (2/15 - ...))
    const float t = __builtin_amdgcn_exp2f(ax * 2.885390081777927f);   // exp(2|x|); inf for |x| > 44: 2/(1+inf) = 0
    const float big = copysignf(1.f - 2.f * __builtin_amdgcn_rcpf(1.f + t), x);
    return ax < 0.35f ? small : big;
}

// fp32 -> bf16, round to nearest even, two at a time (the compiler's cast: v_cvt_pk_bf16_f32) -- the one conversion of the bf16 row
// gathers' shadow rows, of the bf16 halo pack (csrc/elementwise.hip) and of K2's bf16 send epilogues (csrc/gemm.hip)
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {
    typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
    const bf16x2 p = {(__bf16)lo, (__bf16)hi};
    return __builtin_bit_cast(uint32_t, p);
}
// the value of the lane to the right within a pair of lanes (DPP quad_perm [1, 1, 3, 3]; lanes 1 and 3 of a quad read themselves):
// to be called where both lanes of every pair are active
__device__ __forceinline__ float lane_right(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0xF5, 0xF, 0xF, true));
}

// K3/K4 elementwise + loss
hipError_t launch_tanh_backward(uint64_t rows, uint32_t cols, const float *aTg, uint32_t lda,
                                const float *z, uint32_t ldz, float *g, uint32_t ldg, hipStream_t s);
hipError_t launch_tanh_forward(uint64_t rows, uint32_t cols, const float *z, uint32_t ldz, float *h, uint32_t ldh,
                               hipStream_t s);
// softmax + validation stats + maskout quirk + (p - lab)/denom  (CPU_comm.cpp:108-122)
size_t softmax_xent_scratch_bytes(uint32_t cols, uint32_t val_rows);
hipError_t launch_softmax_xent(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz,
                               const float *lab, uint32_t ldl, float *d, uint32_t ldd,
                               float denom, uint32_t val_stt, uint32_t val_end,
                               uint64_t mask_first, uint64_t mask_count, float *stat,
                               float *stat_partial /* 2 * ceil(val_rows/256) floats */, hipStream_t s);
// predictGAT: grad = softmax(z) - lab
hipError_t launch_softmax_sub(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz,
                              const float *lab, uint32_t ldl, float *out, uint32_t ldo, hipStream_t s);
// The send forms of the four producers above (dory_halo_fused_pack_rowwise; elementwise.hip): the tensor as the plain launch leaves
// it, and its rows once more in sd.buf at the slots of sd's map, in sd's wire format (w, bf16, cols; `which` is not read).  *fused =
// true: the rows are in the buffer; false: the plain launch ran instead (no rows, a tensor whose ld is no multiple of 4 in the tanh
// forms).
hipError_t launch_tanh_backward_send(uint64_t rows, uint32_t cols, const float *aTg, uint32_t lda, const float *z, uint32_t ldz, float *g,
                                     uint32_t ldg, const GemmSend &sd, hipStream_t s, bool *fused);
hipError_t launch_tanh_forward_send(uint64_t rows, uint32_t cols, const float *z, uint32_t ldz, float *h, uint32_t ldh, const GemmSend &sd,
                                    hipStream_t s, bool *fused);
hipError_t launch_softmax_xent_send(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab, uint32_t ldl, float *d,
                                    uint32_t ldd, float denom, uint32_t val_stt, uint32_t val_end, uint64_t mask_first, uint64_t mask_count,
                                    float *stat, float *stat_partial, const GemmSend &sd, hipStream_t s, bool *fused);
hipError_t launch_softmax_sub_send(uint32_t rows, uint32_t cols, const float *z, uint32_t ldz, const float *lab, uint32_t ldl, float *out,
                                   uint32_t ldo, const GemmSend &sd, hipStream_t s, bool *fused);
hipError_t launch_fill_uniform(float *d, uint64_t rows, uint32_t cols, uint32_t ld, uint64_t seed,
                               float lo, float hi, hipStream_t s);
hipError_t launch_fill_uniform_ids(float *d, uint64_t rows, uint32_t cols, uint32_t ld,
                                   const uint32_t *row_ids, uint64_t seed, float lo, float hi,
                                   hipStream_t s);
hipError_t launch_onehot(float *d, uint64_t rows, uint32_t cols, uint32_t ld, const uint32_t *labels,
                         hipStream_t s);
hipError_t launch_pad_copy(float *dst, uint32_t ldd, const float *src, uint32_t lds, uint64_t rows,
                           uint32_t cols, hipStream_t s);
hipError_t launch_row_axpy(float *out, const float *S, const float *rs, const float *x /* nullptr: out += rs * S */, uint64_t rows, uint32_t ld,
                           hipStream_t s);
// out = xb + rs * S with xb read from bf16 rows of ld elements (launch_bf16_rows; dory_gat_bf16_gather)
hipError_t launch_row_axpy_bf16(float *out, const float *S, const float *rs, const uint16_t *xb, uint64_t rows, uint32_t ld, hipStream_t s);

// K5 GAT edge kernels
hipError_t launch_edge_forward_gat(uint32_t N, uint32_t F, const uint64_t *colptr, const float *z,
                                   uint32_t ldz, const float *a, float *az, float *A,
                                   float *arow /*N: the column's A value*/, hipStream_t s,
                                   float *azrow = nullptr /*N: the column's az value; az == A == nullptr: per-edge copies left to launch_expand_rows_to_edges*/);
hipError_t launch_expand_rows_to_edges(uint32_t N, const uint64_t *colptr, const float *row, float *out, hipStream_t s);
hipError_t launch_edge_backward_gat(uint32_t N, uint32_t F, const uint64_t *colptr, const float *grad,
                                    uint32_t ldg, const float *az, const float *a, float *dA,
                                    float *cw /*N: deg(v)*dLRelu_v*/, float *drow /*N: the column's dA value*/,
                                    hipStream_t s, const float *azrow = nullptr /*N: read instead of az; dA may then be nullptr*/);
hipError_t launch_rowdot(uint32_t N, uint32_t F, const float *X, uint32_t ld, const float *r, float *y,
                         hipStream_t s);
hipError_t launch_colsum_w(uint32_t N, uint32_t F, const float *X, uint32_t ld, const float *w,
                           float *partial, size_t partial_bytes, float *out, hipStream_t s);

// multi-head GAT extension (csrc/gat_mh.hip)
hipError_t launch_gatmh_scores(uint32_t N, uint32_t K, uint32_t D, const float *z, uint32_t ldz, const float *a_l,
                               const float *a_r, float *el, float *er, uint32_t ldk, hipStream_t s);
// dory_gatmh_bf16_ghosts: the same scores from bf16 rows (a ghost tensor's twin, ldz elements a row) -- the bits launch_gatmh_scores gives
// on the widened rows; the same selection between the two kernels
hipError_t launch_gatmh_scores_bf16(uint32_t N, uint32_t K, uint32_t D, const uint16_t *z, uint32_t ldz, const float *a_l,
                                    const float *a_r, float *el, float *er, uint32_t ldk, hipStream_t s);
hipError_t launch_gatmh_forward(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                const uint32_t *rowidx, const float *z, const float *el, const float *er, float *o,
                                float *m, float *den, hipStream_t s);
// source-blocked forward (statistics pass, weighted sum over K1b's blocked adjacency, reduce + self edge)
hipError_t launch_gatmh_forward_blocked(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk,
                                        const uint64_t *colptr, const uint32_t *rowidx, const BlockedAdj &B,
                                        const float *z, const float *zg /*ghost rows (ids >= N) or nullptr*/,
                                        const float *el, const float *elg, const float *er, float *o, float *m,
                                        float *den, float *partial /*nb x N x ld*/, bool ghosts, hipStream_t s,
                                        float *stat_partial = nullptr /*2 x nb x N x ldk floats: online softmax per block, no statistics pass*/,
                                        const float *a_l = nullptr /*K x D: source scores formed from the gathered rows*/);
// source-blocked backward in two phases (a partitioned run exchanges the ghost rows of dO and st4 in between):
// dst = t, der, st4 = (er, m, 1/den, t) per local (v,k); src = del, dz.  lds4: float4 stride of the st4 rows.
bool gatmh_backward_blocked_ok(uint32_t K, uint32_t D, uint32_t ld);
hipError_t launch_gatmh_backward_blocked_dst(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk,
                                             const BlockedAdj &Bin, const float *z, const float *zg, const float *el,
                                             const float *elg, const float *er, const float *m, const float *den,
                                             const float *d_o, float *t, float *der, float *partial, float4 *st4,
                                             uint32_t lds4, bool ghosts, hipStream_t s,
                                             const float *a_l = nullptr /*K x D: source scores formed from the gathered rows*/);
hipError_t launch_gatmh_backward_blocked_src(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk,
                                             const BlockedAdj &Bout, const float *z, const float *el, const float *d_o,
                                             const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                             const float *der, const float *a_l, const float *a_r, float *del, float *dz,
                                             float *partial /*nb x N x (ld + K) floats*/, bool ghosts, hipStream_t s);
// the edge passes on K1s's skeleton (csrc/gat_mh_sweep.hip): register-resident sums over all source blocks of the sweep layout,
// single-pass softmax against a per-(v,k) upper-bound shift; the destination side of the backward pass needs no edges
inline int gatmh_sweep_group(uint32_t ld) { return ld >= 128 ? 32 : 16; }   // lanes per slab of a row: 128 floats, or one slab of 64
int gatmh_sweep_hl(uint32_t K, uint32_t D, uint32_t ld);   // lanes per head; 0 = shape not covered (blocked kernels)
int gatmh_sweep_rows(const BlockedAdj &S, int group, int HL, int pass /*0 forward, 1 source side*/);   // rows per lane group of a launch
// the wide form of the passes on bf16 rows (option gatmh_bf16_wide; gatmh_*_sweep_bf16x8_kernel): 16-lane groups, two rows per group,
// eight features per lane -- rows of 128 floats or more, several heads of 16 / 32 / 64 features
bool gatmh_wide_applies(uint32_t K, uint32_t D, uint32_t ld);
constexpr int GATMH_WIDE_GROUP = 16, GATMH_WIDE_ROWS = 2;
size_t gatmh_sweep_scratch_bytes(const BlockedAdj &S, uint32_t N, uint32_t ld, uint32_t ldk);
hipError_t launch_gatmh_sweep_begin(uint32_t N, uint32_t G, uint32_t K, uint32_t ld, uint32_t ldk, const BlockedAdj &S, const float *el,
                                    const float *elg, float *scratch, hipStream_t s);
hipError_t launch_gatmh_forward_sweep_part(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const BlockedAdj &S,
                                           const float *z, const float *zg, const float *er, const float *a_l, float *o, float *op,
                                           float *scratch, const SweepPart &p, const float *el, const float *elg /* the sources' scores (local, ghost rows) */);
hipError_t launch_gatmh_forward_sweep_finish(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                             const uint32_t *rowidx, const BlockedAdj &S, const float *z, const float *zg, const float *el,
                                             const float *elg, const float *er, float *o, float *op, float *m, float *den, float *dpos,
                                             float *scratch, hipStream_t s,
                                             bool bf16 = false /* z / zg stay fp32: the self edge's and the recomputed rows' are rounded in registers */);
hipError_t launch_gatmh_dst_rowwise(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const float *d_o, const float *o,
                                    const float *op, const float *dpos, const float *er, const float *m, const float *den, float *t,
                                    float *der, float4 *st4, uint32_t lds4, hipStream_t s);
// dory_gatmh_bwd_merged_exchange, producer-packed: the send form also stores row v's quads of dO below column w and its st records
// (at float offset w + 4k) into the rows row_slots[row_ptr[v] .. row_ptr[v + 1]) of buf, R = w + 4K floats each
// dory_gatmh_halo_bf16 (the launcher's `bf16`; gatmh_dst_rowwise_send_bf16_kernel): the do part is w bf16 (a multiple of 8), the st
// records follow at byte 2 w, R = w / 2 + 4K floats a slot
struct GatmhSend {
    float *buf;
    const uint32_t *row_ptr;     // N + 1 (dory_halo_send_map)
    const uint32_t *row_slots;   // row_ptr[N]
    uint32_t w, R;
};
hipError_t launch_gatmh_dst_rowwise_send(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const float *d_o, const float *o,
                                         const float *op, const float *dpos, const float *er, const float *m, const float *den, float *t,
                                         float *der, float4 *st4, uint32_t lds4, const GatmhSend &sd, hipStream_t s, bool bf16 = false);
size_t gatmh_src_sweep_scratch_bytes(const BlockedAdj &S, uint32_t N, uint32_t G, uint32_t K, uint32_t ld, uint32_t ldk);
hipError_t launch_gatmh_src_sweep_begin(uint32_t N, uint32_t G, uint32_t K, uint32_t ld, uint32_t ldk, const BlockedAdj &S,
                                        const float4 *st4, const float4 *stg, uint32_t lds4, float *scratch, hipStream_t s);
hipError_t launch_gatmh_src_sweep_part(uint32_t N, uint32_t G, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const BlockedAdj &S,
                                       const float *d_o, const float *dog, const float *el, float *dz, float *scratch, const SweepPart &p);
hipError_t launch_gatmh_src_sweep_finish(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const BlockedAdj &S, const float *z,
                                         const float *el, const float *d_o, const float *der, const float *a_l, const float *a_r, float *del,
                                         float *dz, float *scratch, hipStream_t s,
                                         bool bf16 = false /* d_o stays fp32: the self edge's row is rounded in registers */);
// the row-gather family with ghost rows (csrc/gat_mh_rows.hip): one lane group per row, one float4 per lane, ids >= N select row
// id - N of the ghost array (zg / elg / dog / stg: null on a rank without ghosts); any shape of gatmh_shape_ok with K*D <= ld <= 256.
// forward: o, m (the row's true maximum), den, op, dpos; dst: t, der, st4 (an edge pass; where op / dpos are current and
// launch_gatmh_dst_rowwise covers the shape the caller runs that instead); src: del, dz with the finishing terms
bool gatmh_rows_ok(uint32_t K, uint32_t D, uint32_t ld);
// dory_gatmh_row_gather_hub_split: the hub rows of a launch -- the adjacency's chunk plan (Adjacency::hub_rows) and the scratch their
// chunks leave their states in, nchunks x gatmh_rows_hub_state_floats(pass, ld, ldk) floats (pass 0 forward, 1 dst, 2 src).  With
// hubs == nullptr or no chunk in the plan a launcher launches exactly what it launched before the feature.
struct GatmhHubs {
    LongRowsDev plan;
    uint32_t chunk = 0;      // rows with more entries than this are the plan's rows
    float *state = nullptr;
};
size_t gatmh_rows_hub_state_floats(int pass, uint32_t ld, uint32_t ldk);
// dory_gatmh_row_gather_overlap: a launch over n listed rows instead of all N (unit i = row rows[i]; device memory, ids < N).  With a list
// the forward and the source side run their *_list_kernel: the chunk units of `hubs` (if it has any; its hub rows among the listed ones are
// skipped and merged as ever), then the listed rows -- each computed whole by the body of the all-N launch, so it keeps its bits.
struct GatmhRowList {
    const uint32_t *rows = nullptr;
    uint32_t n = 0;
    // false: the launch before the wait -- `hubs` only says which code the listed rows run (the hub kernel's, where the plan has chunks:
    // what computes them with the switch off); no chunk unit, no merge, no row skipped
    bool chunks = true;
};
// what the three launchers gather: fp32 rows; the shadow rows, four bf16 (8 bytes) per lane and edge; or -- dory_gatmh_row_gather_bf16_wide --
// the shadow rows, eight bf16 (16 bytes) per lane and edge on half the lanes per row: the narrow bf16 form's bits.  The wide form
// needs a shape of gatmh_rows8_form (gat_mh_shapes.hpp) and 16-byte aligned rows: gatmh_rows_wide_ok, else the launchers refuse it
// (hipErrorInvalidValue) and the caller runs the narrow form
enum GatmhRowsForm { GATMH_ROWS_FP32 = 0, GATMH_ROWS_BF16 = 1, GATMH_ROWS_BF16_WIDE = 2 };
bool gatmh_rows_wide_ok(uint32_t K, uint32_t D, uint32_t ld, const void *rows, const void *ghost_rows);
hipError_t launch_gatmh_rows_forward(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                     const uint32_t *rowidx, const float *z, const float *zg, const float *el, const float *elg,
                                     const float *er, const float *a_l, float *o, float *op, float *m, float *den, float *dpos,
                                     hipStream_t s, int form = GATMH_ROWS_FP32 /* bf16 forms: z / zg are their shadow rows (launch_bf16_rows) */,
                                     const GatmhHubs *hubs = nullptr, const GatmhRowList *list = nullptr);
hipError_t launch_gatmh_rows_dst(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                 const uint32_t *rowidx, const float *z, const float *zg, const float *el, const float *elg,
                                 const float *er, const float *a_l, const float *m, const float *den, const float *d_o, float *t, float *der,
                                 float4 *st4, uint32_t lds4, hipStream_t s, int form = GATMH_ROWS_FP32 /* bf16 forms: z / zg are their shadow rows */,
                                 const GatmhHubs *hubs = nullptr);
hipError_t launch_gatmh_rows_src(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *rowptr,
                                 const uint32_t *colidx, const float *z, const float *el, const float *d_o, const float *dog,
                                 const float4 *st4, const float4 *stg, uint32_t lds4, const float *der, const float *a_l, const float *a_r,
                                 float *del, float *dz, hipStream_t s, int form = GATMH_ROWS_FP32 /* bf16 forms: d_o / dog are their shadow rows */,
                                 const GatmhHubs *hubs = nullptr, const GatmhRowList *list = nullptr);
// dory_gatmh_row_gather_edge_split: the carry form of the forward and the source side (gatmh_rows_*_carry_kernel).  cy: the adjacency's
// local-first copy (RowsEdgeSplit) and N slots of gatmh_rows_hub_state_floats(0 forward / 2 source side, ld, ldk) floats; walk: both
// ranges of every row in one launch, or the local entries + self edge (FIRST: states parked for the rows with ghost entries) and, after
// the ghost rows have landed, the ghost entries of the boundary rows (SECOND).  BOTH and FIRST + SECOND give the same bits.  form:
// GATMH_ROWS_FP32 or GATMH_ROWS_BF16 (there is no wide carry form)
struct GatmhCarry {
    const uint32_t *idx = nullptr;
    const uint64_t *mid = nullptr;
    const uint32_t *rows = nullptr;
    uint32_t nrows = 0;
    float *state = nullptr;
};
enum GatmhWalk { GATMH_WALK_BOTH = 0, GATMH_WALK_FIRST = 1, GATMH_WALK_SECOND = 2 };
hipError_t launch_gatmh_rows_forward_carry(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr, const float *z,
                                           const float *zg, const float *el, const float *elg, const float *er, const float *a_l, float *o,
                                           float *op, float *m, float *den, float *dpos, hipStream_t s, int form, const GatmhCarry &cy,
                                           int walk);
hipError_t launch_gatmh_rows_src_carry(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *rowptr, const float *z,
                                       const float *el, const float *d_o, const float *dog, const float4 *st4, const float4 *stg, uint32_t lds4,
                                       const float *der, const float *a_l, const float *a_r, float *del, float *dz, hipStream_t s, int form,
                                       const GatmhCarry &cy, int walk);
// row-wise backward (single partition; feature-per-lane or (edge, head, piece)-per-lane kernels by shape)
hipError_t launch_gatmh_backward(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const uint64_t *colptr,
                                 const uint32_t *rowidx, const uint64_t *rowptr, const uint32_t *colidx,
                                 const float *z, const float *el, const float *er, const float *m, const float *den,
                                 const float *d_o, const float *a_l, const float *a_r, float *t, float *del,
                                 float *der, float *dz, float *da_l, float *da_r, float *scratch,
                                 size_t scratch_bytes, hipStream_t s);
hipError_t launch_gatmh_dattn(uint32_t N, uint32_t K, uint32_t D, uint32_t ld, uint32_t ldk, const float *z,
                              const float *del, const float *der, float *da_l, float *da_r, float *scratch,
                              size_t scratch_bytes, hipStream_t s);
hipError_t launch_gatmh_elu(uint64_t rows, uint32_t cols, const float *o, uint32_t ldo, float *h, uint32_t ldh, hipStream_t s);
hipError_t launch_gatmh_elu_bwd(uint64_t rows, uint32_t cols, const float *dh, uint32_t lddh, const float *o,
                                uint32_t ldo, float *d_o, uint32_t lddo, hipStream_t s);
hipError_t launch_gatmh_head_mean(uint64_t rows, uint32_t K, uint32_t C, const float *o, uint32_t ldo, float *logits,
                                  uint32_t ldl, hipStream_t s);
hipError_t launch_gatmh_head_expand(uint64_t rows, uint32_t K, uint32_t C, const float *dl, uint32_t lddl, float *d_o,
                                    uint32_t lddo, hipStream_t s);

// K6 halo pack / unpack
hipError_t launch_gather_rows(float *dst, const float *src, uint32_t ld, uint32_t cols,
                              const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_scatter_rows(float *dst, const float *src, uint32_t ld, uint32_t cols,
                               const uint32_t *rows, uint32_t n, hipStream_t s);
// option halo_exact_rows, cols % 4 != 0: the dense side is one stream of n x cols floats (16-byte aligned), a thread per
// 16-byte quad of it; the scatter also zeroes [cols, ld) of every row it writes.  cols % 4 == 0 < ld takes the kernels
// above with the exact width, and launch_zero_rows_pad after the scatter.
hipError_t launch_gather_rows_exact(float *dst, const float *src, uint32_t ld, uint32_t cols,
                                    const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_scatter_rows_exact(float *dst, const float *src, uint32_t ld, uint32_t cols,
                                     const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_zero_rows_pad(float *dst, uint32_t ld, uint32_t cols, const uint32_t *rows, uint32_t n, hipStream_t s);
// dory_gatmh_bwd_merged_exchange: merged rows [a[v, 0:wa) | b[v, 0:wb)] of wa + wb floats (all widths and lds multiples of 4, the
// dense side 16-byte aligned).  The gather packs the listed rows; the scatter writes whole rows of both tensors: [0, wa) and [0, wb)
// from the stream, zeros into [wa, lda) and [wb, ldb).
hipError_t launch_gather_rows_pair(float *dst, const float *a, uint32_t lda, uint32_t wa, const float *b, uint32_t ldb, uint32_t wb,
                                   const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_scatter_rows_pair(float *a, uint32_t lda, uint32_t wa, float *b, uint32_t ldb, uint32_t wb, const float *src,
                                    const uint32_t *rows, uint32_t n, hipStream_t s);
// dory_gatmh_halo_bf16: the same with the first part as bf16 -- rows of [wa bf16 | wb fp32], wa a multiple of 8 (wa / 2 + wb floats a
// row), lda and ldb multiples of 4.  The gather rounds a[v, 0:wa) to nearest even (pack_bf16x2; the columns behind the tensor's cols
// are its zero padding); the scatter widens them into [0, wa) of a's whole row, zeros into [wa, lda) and [wb, ldb).
hipError_t launch_gather_rows_pair_bf16(float *dst, const float *a, uint32_t lda, uint32_t wa, const float *b, uint32_t ldb, uint32_t wb,
                                        const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_scatter_rows_pair_bf16(float *a, uint32_t lda, uint32_t wa, float *b, uint32_t ldb, uint32_t wb, const float *src,
                                         const uint32_t *rows, uint32_t n, hipStream_t s);
// dory_halo_bf16_rows: the dense side holds rows of row_elems bf16 (a multiple of 4, 8-byte aligned).  The gather rounds
// [0, cols) of every listed row (nearest even, the conversion of launch_bf16_rows) and writes zeros into [cols, row_elems); the
// scatter writes the whole ld-wide row: [0, row_elems) widened from the stream, zeros behind.
hipError_t launch_gather_rows_bf16(void *dst, const float *src, uint32_t ld, uint32_t cols, uint32_t row_elems,
                                   const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_scatter_rows_bf16(float *dst, const void *src, uint32_t ld, uint32_t row_elems,
                                    const uint32_t *rows, uint32_t n, hipStream_t s);
// dory_halo_bf16_ghosts: the received bf16 rows stay bf16.  The keep form of the scatter copies row i of the stream (row_elems bf16, a
// multiple of 4, 8-byte aligned) into row rows[i] of a bf16 twin at stride ld (a multiple of 32: rows of whole 64 bytes), zeros in
// [row_elems, ld) -- the bits rounding the fp32 row launch_scatter_rows_bf16 leaves would give.  The widening is dense: all rows x ld
// elements of a twin into the fp32 tensor of the same shape (n: elements, a multiple of 8; both 16-byte aligned).
hipError_t launch_scatter_rows_bf16_keep(uint16_t *dst, const void *src, uint32_t ld, uint32_t row_elems,
                                         const uint32_t *rows, uint32_t n, hipStream_t s);
hipError_t launch_widen_rows_bf16(float *dst, const uint16_t *src, uint64_t n, hipStream_t s);
// dory_gatmh_bf16_ghosts: the keep form of launch_scatter_rows_pair_bf16 -- the first part of a row [wa bf16 | wb fp32] stays bf16 in row
// rows[i] of a's twin (stride lda elements, a multiple of 8; 16-byte chunks, zeros in [wa, lda)); the second part as the sibling leaves it
hipError_t launch_scatter_rows_pair_bf16_keep(uint16_t *a16, uint32_t lda, uint32_t wa, float *b, uint32_t ldb, uint32_t wb, const float *src,
                                              const uint32_t *rows, uint32_t n, hipStream_t s);
// option halo_direct_recv: whole ld-wide rows (any ld) between the caller-visible order of a ghost tensor and its stored (wire)
// order, off the epoch's path -- to_wire: dst[i] = src[order[i]] (upload), else dst[order[i]] = src[i] (download)
hipError_t launch_permute_rows(float *dst, const float *src, uint32_t ld, const uint32_t *order, uint32_t n, bool to_wire, hipStream_t s);

// scatter messages (include/dorylus_wire.h): every message of a layout into `buf` (16-byte aligned; d_msgs: the layout's table on
// the device, max_rows: its longest message), and a stream of `nrec` records (16-byte aligned, no header) into the ghost rows
uint32_t scatter_msgs_max_cols();
hipError_t launch_scatter_msgs_pack(void *buf, const float *src, uint32_t ld, uint32_t cols, const uint32_t *lvids, const uint32_t *l2g,
                                    const dory_scatter_msg *d_msgs, uint32_t n_msgs, uint32_t max_rows, uint32_t sender, uint32_t layer,
                                    uint32_t dir, hipStream_t s);
hipError_t launch_scatter_msgs_unpack(float *ghost, uint32_t ld, uint32_t cols, const void *records, uint32_t nrec, const uint32_t *gvids,
                                      uint32_t G, const uint32_t *slot_row, uint32_t *stamp, uint32_t round, uint32_t *counts, hipStream_t s);

// K7 Adam
hipError_t launch_adam(float *w, const float *g, float *m, float *v, uint64_t n, float lr_t,
                       hipStream_t s);
hipError_t launch_adam_table(float *w, const float *g, float *m, float *v, uint64_t n, const float *lr_table,
                             const uint32_t *idx, hipStream_t s);
hipError_t launch_bump_counter(uint32_t *idx, hipStream_t s);

}  // namespace dory
