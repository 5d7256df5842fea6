// abi_internal.hpp -- what the translation units of the C-ABI share (abi_context.hip: context, tensor table,
// uploads, options; abi_stages.hip: aggregate / apply_vertex / apply_edge; abi_comm.hip: halo exchange, weight
// update, epoch graph).  Not part of the public interface (include/dorylus_hip.h is).
#ifndef DORY_ABI_INTERNAL_HPP
#define DORY_ABI_INTERNAL_HPP
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>
#include <random>
#include <tuple>

#include "ctx.hpp"

namespace dory {

// records the message for dory_last_error and returns `code`
int fail(dory_ctx *c, int code, const char *fmt, ...);

#define HIPCK(c, call)                                                                 \
    do {                                                                               \
        hipError_t e__ = (call);                                                       \
        if (e__ != hipSuccess)                                                         \
            return fail((c), DORY_ERR_HIP, "%s failed: %s (%s:%d)", #call,             \
                        hipGetErrorString(e__), __FILE__, __LINE__);                   \
    } while (0)
#define NCCLCK(c, call)                                                                \
    do {                                                                               \
        ncclResult_t r__ = (call);                                                     \
        if (r__ != ncclSuccess)                                                        \
            return fail((c), DORY_ERR_COMM, "%s failed: %s (%s:%d)", #call,            \
                        ncclGetErrorString(r__), __FILE__, __LINE__);                  \
    } while (0)
#define CHECK_CTX(c)                                                                   \
    if (!(c)) return DORY_ERR_ARG;                                                     \
    std::lock_guard<std::mutex> lock__((c)->mu);                                       \
    HIPCK((c), hipSetDevice((c)->device))

#define NEED_IN(fn, ptr, l, nm)                                                           \
    Tensor *ptr = find(c, (l), nm);                                                       \
    if (!ptr) return fail(c, DORY_ERR_ARG, "%s: tensor '%s'@%u missing", fn, nm, (unsigned)(l))
#define NEED(ptr, l, nm) NEED_IN(__func__, ptr, l, nm)

// ---- timing: HIP events on the stream the kernels run on --------------------------
// the two events of one timed interval: from c->ev_pool (drain_timing hands them back), or new ones
inline std::pair<hipEvent_t, hipEvent_t> take_event_pair(dory_ctx *c) {
    std::pair<hipEvent_t, hipEvent_t> ev{nullptr, nullptr};
    if (c->ev_pool.empty()) {
        (void)hipEventCreate(&ev.first);
        (void)hipEventCreate(&ev.second);
    } else {
        ev = c->ev_pool.back();
        c->ev_pool.pop_back();
    }
    return ev;
}
struct Timed {
    dory_ctx *c;
    hipStream_t s;
    const char *fam;
    hipEvent_t a = nullptr, b = nullptr;
    Timed(dory_ctx *ctx, const char *family, hipStream_t st) : c(ctx), s(st), fam(family) {
        if (!c->timing || c->capturing) return;
        std::tie(a, b) = take_event_pair(c);
        (void)hipEventRecord(a, s);
    }
    ~Timed() {
        if (!c->timing || c->capturing) return;
        (void)hipEventRecord(b, s);
        c->pending.push_back({fam, a, b});
    }
};
// Overlap bookkeeping (timing on only): the exchange whose ghosts are still landing when the compute stream goes on is
// recorded as family "halo_deferred", the launch that runs beside it (local-source blocks / interior rows) as
// "spmm_beside_halo"; drain_timing intersects the two intervals on the device's clock into "halo_hidden".
// bench.py: multi_gpu.halo_overlap_fraction = halo_hidden / halo_deferred.

void drain_timing(dory_ctx *c);
int alloc_tensor(dory_ctx *c, Tensor &t, uint64_t rows, uint32_t cols);
Tensor *find(dory_ctx *c, uint32_t layer, const char *name);
Tensor *findw(std::vector<std::map<std::string, Tensor>> &tab, uint32_t layer, const char *name);
void free_table(std::vector<std::map<std::string, Tensor>> &tab);
int ensure_scratch(dory_ctx *c, size_t bytes);
// dory_gatmh_row_gather_hub_split: the adjacency's chunk plan for the context's chunk size, built if it is not the cached one (abi_context.hip)
int hub_plan_ensure(dory_ctx *c, dory::Adjacency &A);
// dory_gatmh_row_gather_overlap: the adjacency's rows in launch order (Adjacency::rows_split) for the context's hub chunk size, built if it
// is not the cached one (abi_context.hip)
int interior_plan_ensure(dory_ctx *c, dory::Adjacency &A);
// dory_gatmh_row_gather_edge_split: the adjacency's local-first copy (Adjacency::rows_edge), built if it is not there (never while an
// epoch graph is recording); the buffer of the rows' states between the two launches of a pass, at least `bytes` large
int rows_edge_ensure(dory_ctx *c, dory::Adjacency &A);
int carry_state_ensure(dory_ctx *c, size_t bytes);
// ... and the ghost sources' scores dory_apply_edge left until the exchange of z has landed: launched by wait_halo (abi_stages.hip)
int gatmh_ghost_scores_flush(dory_ctx *c);
// c->partial (K1b's partial rows, the sweeps' gate counters); `what` names it in the refusal inside a recording
int ensure_partial(dory_ctx *c, size_t bytes, const char *what);
int ensure_sweep(dory_ctx *c, Adjacency &A, int group);
int k1s_rows(dory_ctx *c, const BlockedAdj &S, int group /* the wide form: 16 */);   // K1s's rows per lane group on the layout S (abi_stages.hip)
// drops a recorded epoch (hipGraph): anything that frees or moves what the recorded kernels point at calls this
void epoch_graph_drop_locked(dory_ctx *c);
std::vector<uint32_t> degree_order(const uint64_t *ptr, uint32_t N);
int gemm(dory_ctx *c, int ta, int tb, uint32_t M, uint32_t N, uint32_t K, const Tensor &A, const Tensor &B, Tensor &C,
         Tensor *C2 = nullptr);

template <typename T>
int upload_array(dory_ctx *c, T **dst, const T *src, uint64_t n) {
    size_t b = n * sizeof(T);
    HIPCK(c, hipMalloc((void **)dst, b ? b : 256));
    if (b) HIPCK(c, hipMemcpy(*dst, src, b, hipMemcpyHostToDevice));
    return DORY_OK;
}

// Ghost rows of the last halo exchange land on the comm stream; with "halo_overlap" the compute stream is only
// made to wait for them (event ev_b) by the first consumer (abi_comm.hip).
int wait_halo(dory_ctx *c);
// in-process device transport: second half of a deferred exchange (abi_comm.hip); wait_halo and dory_sync run it
int local_exchange_finish(dory_ctx *c);
// GAT prototype, lazy per-edge tensors (ctx.hpp): bring az@layer (1), "A" (2), dA@layer (4) up to date before somebody reads them
int gat_materialize(dory_ctx *c, uint32_t layer, int which);
// transform-first order applies to this GCN layer (option, model shape, adjacency values): see abi_context.hip
bool tf_layer(dory_ctx *c, uint32_t layer);
bool tf_active(dory_ctx *c);   // = tf_layer(c, 0)
// one all-to-all-v of rows with the plan of `dir` (abi_comm.hip)
// follows_rule == false: rows whose element the rule of dory_halo_bf16_rows does not decide (the multi-head GAT's st: always fp32)
int exchange_rows(dory_ctx *c, int dir, Tensor *src, Tensor *ghost, bool defer, const RowPair *pair = nullptr /* merged rows: ctx.hpp */,
                  bool follows_rule = true);
// dory_gatmh_bwd_merged_exchange (abi_comm.hip).  gatmh_bwd_exchange: the ghost destinations' do and st rows between the two phases of
// a whole backward sweep -- one exchange of merged rows where the switch, the transport and the plan allow it, else the two exchanges
// (a counted split fallback while the switch is on).  gatmh_bwd_send_target: asked before the destination side's row-wise kernel is
// launched -- *send: that kernel may write the merged send rows itself (the merged exchange will be taken, dory_halo_fused_pack is on,
// the backward plan has its send map, no recording, the send buffer holds them); then *sd is filled in and the previous exchange has
// finished reading the buffer.  Producer and exchange sit inside one dory_aggregate call: no stamp.
// defer_last (dory_gatmh_row_gather_overlap, the row-gather family; the sweep and blocked forms pass false): the LAST exchange of the pass
// -- the merged one, or st's in the two-exchange case -- is issued deferred where option halo_overlap is set; the caller calls wait_halo
// before it reads bg_do / bg_st and before it returns.  do's exchange, the first of two, is never deferred: exchange_rows and the local
// transport hold ONE pending exchange.
int gatmh_bwd_exchange(dory_ctx *c, Tensor *dO, Tensor *bgdo, Tensor *st, Tensor *bgst, bool producer_packed, bool defer_last = false);
// *bf16 (dory_gatmh_halo_bf16): the do part of those rows is bf16 by the rule of this moment -- the launcher's bf16 send form.
int gatmh_bwd_send_target(dory_ctx *c, const Tensor *dO, const Tensor *st, GatmhSend *sd, bool *send, bool *bf16);
uint32_t gatmh_merged_row_max(const dory_ctx *c);
// The fused halo pack (abi_comm.hip).  fused_pack_target: the GEMM about to write `out` (M rows, the product's C or its tanh output)
// may store its rows into the send buffer too -- the feature is on, a plan and its map exist, `out` is the source of an exchange
// of this model (the resolver halo_tensors uses), nothing of section "not taken" of dorylus_hip.h applies -- then *sd (but `which`)
// and *dir are filled in.  fused_pack_stamp: that GEMM has been enqueued (`rowwise`: a row-wise producer's send form instead,
// dory_halo_fused_pack_rowwise, which asks fused_pack_target the same question about the tensor it writes).  fused_stamp_drop: whatever the stamp named may be stale.
bool fused_pack_target(dory_ctx *c, const Tensor *out, uint32_t M, GemmSend *sd, int *dir);
void fused_pack_stamp(dory_ctx *c, const Tensor *out, int dir, const GemmSend &sd, bool rowwise = false);
inline void fused_stamp_drop(dory_ctx *c) { c->fused_stamp = FusedStamp(); }
// something other than a fusing GEMM writes `t` (may be null): a stamp that names it no longer describes its rows
inline void fused_note_write(dory_ctx *c, const Tensor *t) { if (t && c->fused_stamp.src == t) fused_stamp_drop(c); }
// bf16 ghost twins (dory_halo_bf16_ghosts; abi_comm.hip).  ghost_fp32_current: somebody is about to read the fp32 rows of `t` (may be
// null) -- where only its twin is current (DORY_GHOST_TWIN) the exchange in flight is waited for and the twin widened into the fp32
// rows on the compute stream (then DORY_GHOST_BOTH, counted); anything else: nothing.  ghost_wrote_fp32: fp32 rows have been written
// into `t`, all of them.  ghost_twins_alloc: with the switch on, a twin for every tensor the rule of dory_halo_bf16_rows can cover
// that has none yet (GCN: fg of layers >= 1, fgxw, bg, bgg; GAT prototype: fg_z, bg_d; the multi-head GAT with dory_gatmh_bf16_ghosts:
// fg_z, bg_do; ld >= 4) -- never inside an epoch.
int ghost_fp32_current(dory_ctx *c, Tensor *t);
inline void ghost_wrote_fp32(Tensor *t) { if (t) t->twin_state = DORY_GHOST_FP32; }
int ghost_twins_alloc(dory_ctx *c);
// dory_gatmh_bf16_ghosts: the exchange of do -> bg_do that a whole backward pass is about to make (gatmh_bwd_exchange, merged or not)
// will leave its rows in bg_do's twin, by the settings of this moment -- what the reservation of the shadow rows asks before that exchange
bool gatmh_do_lands_in_twin(const dory_ctx *c, const Tensor *dO, const Tensor *bgdo);
// scatter messages (abi_comm.hip): everything dory_ctx::scatter owns, at dory_destroy
void scatter_free(dory_ctx *c);
// K1b bookkeeping (abi_stages.hip)
int ensure_blocked(dory_ctx *c, Adjacency &A, int group, bool narrow_set = false /* the multi-head GAT contexts' second copy (Adjacency::blk16) */);
int blk_group_for(dory_ctx *c, uint32_t ld);
// dory_gat_bf16_gather: the bf16 shadow rows of the model's largest aggregation, reserved outside a recording (abi_stages.hip)
int gat_bf16_reserve_all(dory_ctx *c);

}  // namespace dory
#endif
