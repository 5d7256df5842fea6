// abi_comm.hip -- C-ABI, part 3: ghost-vertex halo exchange (plan, one wire-format record for a packed row, one arm per
// transport: caller's host callbacks / in-process device transport / RCCL all-to-all-v, pack / unpack for foreign
// transports), all-reduce over the same transports for the weight gradients + Adam and for the validation statistics, and
// the epoch graph (hipGraph record / replay); and the one setter path of the feature switches (switches.hpp: switch_set, their
// hooks, switch_stats).  Layout: helpers in dependency order (file-local ones, then the four that abi_internal.hpp declares),
// then the extern "C" entry points.
#include <chrono>
#include <thread>

#include "../../include/dorylus_host.h"
#include "../../include/dorylus_wire.h"
#include "abi_internal.hpp"

using namespace dory;

namespace {

// ---- which transport carries the bytes: the caller's host callbacks (dense rows, or the reference's scatter messages), else the
// in-process group, else RCCL ----------------
enum class Transport { Host, Scatter, Local, Rccl, None };
Transport transport_of(const dory_ctx *c) {
    if (c->scatter.fn && c->tx_ar) return Transport::Scatter;   // (dory_comm_set_scatter_transport: it clears tx_a2a)
    if (c->tx_a2a && c->tx_ar) return Transport::Host;   // (dory_comm_set_host_transport sets both or none)
    if (c->local) return Transport::Local;
    return c->nccl ? Transport::Rccl : Transport::None;
}

// ---- timing ---------------------------------------------------------------------------------------------------------------
// an interval for dory_timing_get whose end is recorded by a later call: entry pushed now (order of `pending` = order of
// the first events), end event handed back
void timed_open(dory_ctx *c, const char *fam, hipStream_t s, hipEvent_t *end_out) {
    *end_out = nullptr;
    if (!c->timing || c->capturing) return;
    const auto ev = take_event_pair(c);
    (void)hipEventRecord(ev.first, s);
    c->pending.push_back({fam, ev.first, ev.second});
    *end_out = ev.second;
}

// ---- the wire format of a packed row --------------------------------------------------------------------------------------
// Option halo_exact_rows: a packed row holds exactly `cols` floats instead of the padded `ld` -- what the reference ships
// (featDim floats per row, engine/utils.cpp:623-650).  Every pack and unpack of this file goes through row_wire, pack_rows
// and unpack_rows.
inline bool halo_exact(const dory_ctx *c) { return c->halo_exact.load(std::memory_order_acquire) == 1; }
// Option halo_direct_recv: ghost rows are stored in wire order (received row r at ghost row r), so an exchange whose wire
// width is the ghost tensor's ld lands in the tensor itself -- no receive buffer, no unpack.  Rows narrower than ld
// (halo_exact_rows with cols < ld) are strided in the tensor: they keep the receive buffer and the unpack kernels, which then
// scatter by an identity list (HaloPlan::d_unpack_slots).
inline bool halo_direct(const dory_ctx *c) { return c->halo_direct.load(std::memory_order_acquire) == 1; }
// dory_halo_bf16_ghosts: received bf16 rows stay bf16 in the ghost tensor's twin (`keeps`); then an exchange lands directly where
// the wire's row is the twin's -- compared in elements (fp32 rows in an fp32 tensor, bf16 rows in a bf16 twin).  bf16 rows never
// land in fp32 rows.
inline bool keeps_bf16(const dory_ctx *c, RowWire wire, const Tensor *ghost) { return wire.bf16 && sw_on(c, SW_HALO_BF16_GHOSTS) && ghost && ghost->twin; }
inline bool lands_directly(const HaloPlan &p, RowWire wire, uint32_t ghost_ld, bool keep) { return p.direct && wire.w == ghost_ld && wire.bf16 == keep; }
const char *const NO_RECV_BUF = "halo_direct_recv: this exchange needs the receive buffer (rows of %u floats in a tensor of ld %u) and "
                                "dory_halo_plan allocated none: set halo_exact_rows = 1 before dory_halo_plan";

// The record for the rows `who` packs from `src` (pack == true: its width travels) or unpacks into `ghost` (pack == false);
// the tensor of the other end may be null (the *_tensor entry points know one only), `buf` is a caller's buffer or null.
// The padded row width travels (keeps 16-B lanes), or, with option halo_exact_rows, exactly the tensor's columns -- then
// both ends must have the same, and a caller's buffer of rows whose width is no multiple of 4 is addressed in 16-byte quads
// of the whole stream.
// dory_halo_bf16_rows: `rule_dir` is the direction of the exchange whose rule decides the element (wire_bf16, below), or -1 for rows
// whose consumer is unknown (the *_tensor entry points: fp32).  bf16 rows hold the width rounded up to a multiple of 4 elements
// (zeros behind the tensor's cols): multiples of 8 bytes, in a buffer aligned to 8.
inline uint32_t wire_width(const dory_ctx *c, const Tensor *rows) { return halo_exact(c) ? rows->cols : rows->ld; }
bool wire_bf16(const dory_ctx *c, int dir, uint32_t ld);
// the shape alone, without the checks of a buffer: what row_wire fills in and what fused_pack_target sizes the send rows by
inline RowWire wire_shape(const dory_ctx *c, const Tensor *rows, int rule_dir) {
    RowWire out;
    out.exact = halo_exact(c);
    out.w = wire_width(c, rows);
    out.bf16 = rule_dir >= 0 && wire_bf16(c, rule_dir, rows->ld);
    if (out.bf16) {
        out.cols = rows->cols;
        out.w = (out.w + 3u) & ~3u;
    }
    return out;
}
int row_wire(dory_ctx *c, const char *who, const Tensor *src, const Tensor *ghost, bool pack, const void *buf, int rule_dir, RowWire *out) {
    const Tensor *rows = pack ? src : ghost;
    if (halo_exact(c) && src && ghost && src->cols != ghost->cols)
        return fail(c, DORY_ERR_ARG, "%s: widths of source (%u) and ghost tensor (%u) differ", who, src->cols, ghost->cols);
    *out = wire_shape(c, rows, rule_dir);
    if (out->bf16) {
        if ((uintptr_t)buf & 7) return fail(c, DORY_ERR_ARG, "%s: dory_halo_bf16_rows needs an 8-byte aligned buffer", who);
        return DORY_OK;
    }
    if (out->exact && (out->w & 3) && ((uintptr_t)buf & 15))
        return fail(c, DORY_ERR_ARG, "%s: halo_exact_rows with rows of %u floats needs a 16-byte aligned buffer", who, out->w);
    return DORY_OK;
}

// dory_gatmh_bwd_merged_exchange: the merged row [do[v, 0:w) | st[v, 0:4K)] -- w = ld floats of do, or with halo_exact_rows its cols
// rounded up to a multiple of 4 (the columns past cols are the tensor's zero padding, as in the bf16 rows' rule); R = w + 4K is a
// multiple of 4, so every row starts on a 16-byte boundary.
// dory_gatmh_halo_bf16 (`do16`: the rule says bf16 for do at this moment, gatmh_do_bf16 below): the do part as bf16, the exact width
// rounded up to a multiple of 8 -- st starts on a 16-byte boundary, the row is w / 2 + 4K floats, a multiple of 4; st stays fp32
inline RowWire pair_wire(const dory_ctx *c, const Tensor *rows, const Tensor *rows2, bool do16) {
    RowWire out;
    out.exact = halo_exact(c);
    out.bf16 = do16 && !(rows->ld & 7);
    const uint32_t up = out.bf16 ? 7u : 3u;
    out.w = out.exact ? std::min((rows->cols + up) & ~up, rows->ld) : rows->ld;
    out.cols = out.bf16 ? rows->cols : 0;
    out.w2 = rows2->cols;
    return out;
}
// the element kind of the do part of the multi-head GAT's backward rows at this moment: the rule and the arms that keep fp32
inline bool gatmh_do_bf16(const dory_ctx *c, const Tensor *dO) { return c->gnn == DORY_GATMH && wire_bf16(c, DORY_BACKWARD, dO->ld); }

// dory_halo_bf16_rows: an eager exchange or pack that ships fp32 rows while the switch is on (section "not taken" of dorylus_hip.h)
inline void fp32_while_on(dory_ctx *c) {
    if (!c->capturing && sw_on(c, SW_HALO_BF16_ROWS)) c->count[CNT_HALO_FP32_PACKS_WHILE_ON]++;
}
// the plan's send rows of `src`, dense at the wire's width, into dst; counted (eager calls); merged rows (wire.w2): those of src2 behind them
int pack_rows(dory_ctx *c, float *dst, const Tensor *src, RowWire wire, const HaloPlan &p, hipStream_t s, const Tensor *src2 = nullptr) {
    if (dst == c->send_buf) fused_stamp_drop(c);   // (the fused halo pack: whatever a GEMM left in the internal buffer is overwritten)
    if (wire.w2 && wire.bf16) HIPCK(c, launch_gather_rows_pair_bf16(dst, src->d, src->ld, wire.w, src2->d, src2->ld, wire.w2, p.d_send_lvids, p.send_total, s));
    else if (wire.w2) HIPCK(c, launch_gather_rows_pair(dst, src->d, src->ld, wire.w, src2->d, src2->ld, wire.w2, p.d_send_lvids, p.send_total, s));
    else if (wire.bf16) HIPCK(c, launch_gather_rows_bf16(dst, src->d, src->ld, wire.cols, wire.w, p.d_send_lvids, p.send_total, s));
    else if (wire.exact && (wire.w & 3)) HIPCK(c, launch_gather_rows_exact(dst, src->d, src->ld, wire.w, p.d_send_lvids, p.send_total, s));
    else HIPCK(c, launch_gather_rows(dst, src->d, src->ld, wire.w, p.d_send_lvids, p.send_total, s));
    if (!c->capturing) {
        c->halo_rows_packed += p.send_total;
        c->halo_floats_packed += (uint64_t)p.send_total * (wire.row_bytes() / sizeof(float));   // (bf16 rows: 4-byte units, w / 2 a row)
        if (wire.exact && (wire.bf16 ? wire.cols : wire.w) < src->ld) c->halo_exact_packs++;
        if (wire.bf16) { c->count[CNT_HALO_BF16_PACKS]++; c->count[CNT_HALO_BF16_BYTES] += (uint64_t)p.send_total * wire.row_bytes(); }
        else fp32_while_on(c);
    }
    return DORY_OK;
}
// The send rows of an exchange into c->send_buf.  The fused halo pack: they are there already when the stamp names this source,
// direction, element kind (dory_halo_fused_pack_bf16: and the columns that hold values), width and buffer as the wire of this moment
// has them -- the producer's epilogue wrote them -- and then no kernel runs and the stamp is consumed; with the
// feature on every other exchange is a counted fallback (`may_fuse` false: an arm that never takes them, section "not taken" of
// dorylus_hip.h).
// dory_gatmh_bwd_merged_exchange (`pair`): the producer wrote the merged rows inside this very call of dory_aggregate -- no stamp --
// or the pair kernel packs them; the fused pack counts the one as a fused exchange, the other as a fallback.
int send_rows(dory_ctx *c, const Tensor *src, int dir, RowWire wire, const HaloPlan &p, hipStream_t s, bool may_fuse, const RowPair *pair = nullptr) {
    if (wire.bf16 && c->gnn == DORY_GATMH && !c->capturing) {   // (dory_gatmh_halo_bf16_stats: z forward; do backward, alone or in a merged row)
        if (dir == DORY_FORWARD) c->count[CNT_GATMH_FWD_BF16_EXCHANGES]++;
        else {
            c->count[CNT_GATMH_BWD_BF16_EXCHANGES]++;
            c->count[CNT_GATMH_BWD_BF16_ROWS] += p.send_total;
            if (pair && pair->producer_packed) c->count[CNT_GATMH_PRODUCER_PACKED_BF16]++;
        }
    }
    if (pair) {
        if (!c->capturing) {
            c->count[CNT_MERGED_EXCHANGES]++;
            c->count[CNT_MERGED_ROWS] += p.send_total;
            if (pair->producer_packed) c->count[CNT_MERGED_PRODUCER_PACKED]++;
            if (sw_on(c, SW_HALO_FUSED_PACK)) {
                if (pair->producer_packed) { c->count[CNT_FUSED_EXCHANGES]++; c->count[CNT_FUSED_ROWS] += p.send_total; }
                else c->count[CNT_FALLBACK_EXCHANGES]++;
            }
        }
        if (!pair->producer_packed) return pack_rows(c, c->send_buf, src, wire, p, s, pair->src2);
        if (wire.bf16 && !c->capturing) {   // (what travelled as bf16 is counted as for a pack: the merged row with all its bytes)
            c->count[CNT_HALO_BF16_PACKS]++;
            c->count[CNT_HALO_BF16_BYTES] += (uint64_t)p.send_total * wire.row_bytes();
        }
        if (!wire.bf16) fp32_while_on(c);
        return DORY_OK;
    }
    if (sw_on(c, SW_HALO_FUSED_PACK)) {
        const FusedStamp &st = c->fused_stamp;
        if (may_fuse && st.src == src && st.dir == dir && st.bf16 == wire.bf16 && (!wire.bf16 || st.cols == wire.cols) && st.w == wire.w &&
            st.buf == c->send_buf) {
            const bool rowwise = st.rowwise;
            fused_stamp_drop(c);
            if (!c->capturing) {
                c->count[CNT_FUSED_EXCHANGES]++;
                c->count[CNT_FUSED_ROWS] += p.send_total;
                if (rowwise) {   // (dory_halo_fused_pack_rowwise: a row-wise producer wrote them -- counted besides)
                    c->count[CNT_ROWWISE_EXCHANGES]++;
                    c->count[CNT_ROWWISE_ROWS] += p.send_total;
                }
                if (wire.bf16) {   // (what travelled as bf16 is counted as for a pack: a foreign transport sizes by it)
                    c->count[CNT_FUSED_BF16_EXCHANGES]++;
                    c->count[CNT_FUSED_BF16_ROWS] += p.send_total;
                    c->count[CNT_HALO_BF16_PACKS]++;
                    c->count[CNT_HALO_BF16_BYTES] += (uint64_t)p.send_total * wire.row_bytes();
                }
            }
            if (!wire.bf16) fp32_while_on(c);
            return DORY_OK;
        }
        if (!c->capturing) c->count[CNT_FALLBACK_EXCHANGES]++;
    }
    return pack_rows(c, c->send_buf, src, wire, p, s);
}
// the received rows, dense at the wire's width w, into the plan's ghost slots (option halo_direct_recv: row r into ghost row r);
// the exact form writes the whole row: [0, w) from the buffer, zeros into [w, ld) -- the bits the padded form leaves, whatever
// the padding held before
// dory_halo_bf16_ghosts (`twin` not null: the rows are bf16 and stay bf16): the keep form copies them into the twin's rows instead,
// zeros in [w, ld); `ghost` is not touched
// merged rows (wire.w2): whole rows of both ghost tensors, ghost2 at stride ld2 behind the first (`twin`: the first part into the twin's rows)
int unpack_rows(dory_ctx *c, float *ghost, uint32_t ld, RowWire wire, const float *buf, const HaloPlan &p, hipStream_t s, uint16_t *twin = nullptr,
                float *ghost2 = nullptr, uint32_t ld2 = 0) {
    if (wire.w2 && wire.bf16 && twin) {   // (dory_gatmh_bf16_ghosts: the do part stays bf16 in bg_do's twin, st as below)
        HIPCK(c, launch_scatter_rows_pair_bf16_keep(twin, ld, wire.w, ghost2, ld2, wire.w2, buf, p.d_unpack_slots, p.recv_total, s));
    } else if (wire.w2 && wire.bf16) {
        HIPCK(c, launch_scatter_rows_pair_bf16(ghost, ld, wire.w, ghost2, ld2, wire.w2, buf, p.d_unpack_slots, p.recv_total, s));
    } else if (wire.w2) {
        HIPCK(c, launch_scatter_rows_pair(ghost, ld, wire.w, ghost2, ld2, wire.w2, buf, p.d_unpack_slots, p.recv_total, s));
    } else if (twin) {
        HIPCK(c, launch_scatter_rows_bf16_keep(twin, buf, ld, wire.w, p.d_unpack_slots, p.recv_total, s));
    } else if (wire.bf16) {   // (the whole ld-wide row: widened values, zeros behind them)
        HIPCK(c, launch_scatter_rows_bf16(ghost, buf, ld, wire.w, p.d_unpack_slots, p.recv_total, s));
    } else if (wire.exact && (wire.w & 3)) {
        HIPCK(c, launch_scatter_rows_exact(ghost, buf, ld, wire.w, p.d_unpack_slots, p.recv_total, s));
    } else {
        HIPCK(c, launch_scatter_rows(ghost, buf, ld, wire.w, p.d_unpack_slots, p.recv_total, s));
        if (wire.exact && wire.w < ld) HIPCK(c, launch_zero_rows_pad(ghost, ld, wire.w, p.d_unpack_slots, p.recv_total, s));
    }
    return DORY_OK;
}

// dory_halo_bf16_ghosts: all rows of `ghost` have been enqueued on stream s -- fp32 rows (state FP32), or (keep) bf16 rows in its twin:
// counted (eager calls) as landed in the twin itself or copied there by the keep kernel; state TWIN, or, where the tensor's raw
// pointer is out (the caller reads fp32 rows behind the library's back), widened at once behind them on s (widen_now; the deferred
// half of the local transport does it itself, LocalPending::widen_to) and BOTH
// (dory_gatmh_bf16_ghosts_stats: `dir` and `merged` say which of the multi-head GAT's tensors it is -- fg_z, bg_do alone, bg_do of a merged row)
int ghost_rows_landed(dory_ctx *c, Tensor *ghost, bool keep, bool direct, hipStream_t s, bool widen_now, int dir, bool merged = false) {
    if (!keep) { ghost_wrote_fp32(ghost); return DORY_OK; }
    if (!c->capturing) (direct ? c->count[CNT_GHOST_LANDED_DIRECT] : c->count[CNT_GHOST_LANDED_BY_KERNEL]) += 1;
    if (!c->capturing && c->gnn == DORY_GATMH) (dir == DORY_FORWARD ? c->count[CNT_GATMH_TWIN_FWD] : merged ? c->count[CNT_GATMH_TWIN_BWD_MERGED] : c->count[CNT_GATMH_TWIN_BWD]) += 1;
    ghost->twin_state = ghost->raw_handed ? DORY_GHOST_BOTH : DORY_GHOST_TWIN;
    if (ghost->raw_handed && widen_now) HIPCK(c, launch_widen_rows_bf16(ghost->d, ghost->twin, ghost->rows * ghost->ld, s));
    return DORY_OK;
}

// the four split entry points (foreign transports, multi-context tests) after their own checks: pack the plan's send rows of
// `src` into the caller's buffer, or unpack it into `ghost` (dory_halo_bf16_ghosts: into its twin, by the exchange's rule); the
// other tensor is the one halo_tensors resolved, or null
int split_rows(dory_ctx *c, const char *who, bool pack, int dir, const Tensor *src, Tensor *ghost, float *buf, bool follows_rule) {
    RowWire wire;
    int rc = row_wire(c, who, src, ghost, pack, buf, follows_rule ? dir : -1, &wire);
    if (rc) return rc;
    Timed t(c, "halo", c->compute);
    if (pack) return pack_rows(c, buf, src, wire, c->plan[dir], c->compute);
    const bool keep = keeps_bf16(c, wire, ghost);
    if (ghost->rows != c->plan[dir].recv_total && keep)   // (the twin holds exactly the plan's rows)
        return fail(c, DORY_ERR_ARG, "%s: ghost tensor of %llu rows for a plan that receives %u", who, (unsigned long long)ghost->rows, c->plan[dir].recv_total);
    rc = unpack_rows(c, ghost->d, ghost->ld, wire, buf, c->plan[dir], c->compute, keep ? ghost->twin : nullptr);
    return rc ? rc : ghost_rows_landed(c, ghost, keep, false, c->compute, true, dir);
}

// resolve (layer, dir) -> source tensor, ghost tensor, as Engine::scatterGCN/GAT do; false: layer out of range.  No side effects:
// halo_tensors (every exchange and split entry point) and fused_pack_target (which GEMM outputs travel) both read this one table.
bool halo_route(dory_ctx *c, uint32_t layer, int dir, Tensor **src, Tensor **ghost) {
    *src = *ghost = nullptr;
    if (c->gnn == DORY_GCN && dir == DORY_BACKWARD && tf_layer(c, layer)) {
        *src = find(c, layer, "g");      // transform-first: A^T g_l needs the ghost rows of g_l
        *ghost = find(c, layer, "bgg");
    } else if (c->gnn == DORY_GCN && dir == DORY_FORWARD && layer > 0 && tf_layer(c, layer)) {
        *src = find(c, layer, "xw");     // transform-first: the already transformed (narrower) rows travel
        *ghost = find(c, layer, "fgxw");
    } else if (c->gnn == DORY_GCN) {
        if (layer == 0 || layer >= c->L) return false;
        if (dir == DORY_FORWARD) { *src = find(c, layer - 1, "h"); *ghost = find(c, layer, "fg"); }   // gcn_ops.cpp:205-214
        else { *src = find(c, layer, "grad"); *ghost = find(c, layer - 1, "bg"); }
    } else {
        if (layer == 0 || layer > c->L) return false;
        if (dir == DORY_FORWARD) { *src = find(c, layer - 1, "z"); *ghost = find(c, layer - 1, "fg_z"); }   // gat_ops.cpp:277-287
        else { *src = find(c, layer - 1, "grad"); *ghost = find(c, layer - 1, "bg_d"); }
    }
    return true;
}
// dory_halo_bf16_rows, the rule: with the switch on, an exchange ships bf16 rows iff the aggregation that reads its ghost tensor gathers
// bf16 rows under the settings of this moment -- GCN (fg / fgxw forward, bg / bgg backward): option gcn_bf16_gather >= 1 forward, == 2
// backward; GAT prototype (fg_z, bg_d): dory_gat_bf16_gather's mode likewise; the multi-head GAT only with dory_gatmh_halo_bf16 on top:
// then option gatmh_bf16_gather likewise (z -> fg_z forward; backward: the do of the sweep's own exchange -- with the option set its
// sweeps, and with dory_gatmh_row_gather_bf16 the row-gather family, gather fg_z / bg_do from rounded copies only, and the blocked forms
// that read them in fp32 are refused; the family's destination-side edge pass of a layer whose forward swept reads fg_z in fp32).  The same for every
// layer of a model.  Reads atomics only: the peers of the local transport ask it of each other.
bool halo_ships_bf16(const dory_ctx *c, int dir) {
    if (!sw_on(c, SW_HALO_BF16_ROWS)) return false;
    if (c->gnn == DORY_GATMH && !sw_on(c, SW_GATMH_HALO_BF16)) return false;
    const int mode = (c->gnn == DORY_GCN ? c->gcn_bf16_mode : c->gnn == DORY_GATMH ? c->gatmh_bf16_mode_pub : c->gat_bf16_mode_pub).load(std::memory_order_acquire);
    return mode >= (dir == DORY_FORWARD ? 1 : 2);
}
// ... and what keeps fp32 although the rule says yes: the scatter-message transport (the reference's format), and a plan made with
// halo_direct_recv = 1 (a 16-bit row cannot land in an fp32 ghost tensor, and such a plan may have no receive buffer) -- unless
// dory_halo_bf16_ghosts is on and the tensor (ld: the same number on every rank) has a twin for them to land in.  direct_keeps: that
// exception, from settings every rank can read of every other.
// (the multi-head GAT has twins only with dory_gatmh_bf16_ghosts on top: without it its direct plans keep fp32)
inline bool direct_keeps(const dory_ctx *c, uint32_t ld) { return sw_on(c, SW_HALO_BF16_GHOSTS) && ld >= 4 && (c->gnn != DORY_GATMH || sw_on(c, SW_GATMH_BF16_GHOSTS)); }
bool wire_bf16(const dory_ctx *c, int dir, uint32_t ld) {
    return halo_ships_bf16(c, dir) && (!c->plan[dir].direct || direct_keeps(c, ld)) && transport_of(c) != Transport::Scatter;
}
int halo_tensors(dory_ctx *c, uint32_t layer, int dir, Tensor **src, Tensor **ghost) {
    if (!halo_route(c, layer, dir, src, ghost)) return fail(c, DORY_ERR_ARG, "halo: layer %u out of range", layer);
    // fg_z is about to change: the kept neighbour sum no longer holds
    if (c->gnn != DORY_GCN && dir == DORY_FORWARD && layer - 1 < c->gat_nsum_valid.size()) c->gat_nsum_valid[layer - 1] = 0;
    if (!*src || !*ghost) return fail(c, DORY_ERR_ARG, "halo: tensors missing");
    return DORY_OK;
}
// multi-head extension: the backward sweep exchanges dO and its per-vertex statistics itself, between its two phases
// (dory_aggregate); the scatter stage of the reference's GAT order has nothing to ship before it
inline bool exchange_skipped(const dory_ctx *c, int dir) { return c->gnn == DORY_GATMH && dir == DORY_BACKWARD; }

// ---- the fused halo pack: the plan's send list turned round, on the device (HaloPlan::d_send_map) -------------------------------
int build_send_map(dory_ctx *c, HaloPlan &p, const uint32_t *send_lvids) {
    std::vector<uint32_t> map((size_t)c->N + 1 + p.send_total);
    if (dory_halo_send_map(c->N, c->numNodes, p.send_counts.data(), send_lvids, map.data(), map.data() + c->N + 1))
        return fail(c, DORY_ERR_ARG, "halo_fused_pack: %s", dory_host_last_error());
    if (p.d_send_map) (void)hipFree(p.d_send_map);
    p.d_send_map = nullptr;
    p.send_map_rows = c->N;
    return upload_array(c, &p.d_send_map, map.data(), map.size());
}

// ---- the pack / receive buffers -------------------------------------------------------------------------------------------
int grow_buffer(dory_ctx *c, float **buf, size_t *cap, size_t bytes) {
    if (bytes <= *cap) return DORY_OK;
    if (*buf) (void)hipFree(*buf);
    *buf = nullptr; *cap = 0;
    HIPCK(c, hipMalloc((void **)buf, bytes));
    *cap = bytes;
    return DORY_OK;
}
// c->send_buf / c->recv_buf hold at least that much: one device-wide synchronisation if either grows, then free, then malloc
int ensure_exchange_buffers(dory_ctx *c, size_t send_bytes, size_t recv_bytes) {
    if (send_bytes > c->send_cap || recv_bytes > c->recv_cap) HIPCK(c, hipDeviceSynchronize());
    if (send_bytes > c->send_cap) fused_stamp_drop(c);   // (the fused halo pack: the rows a GEMM left go with the old buffer)
    int rc = grow_buffer(c, &c->send_buf, &c->send_cap, send_bytes);
    return rc ? rc : grow_buffer(c, &c->recv_buf, &c->recv_cap, recv_bytes);
}

// ---- scatter messages (include/dorylus_wire.h: the reference's own graph-server <-> graph-server wire) -------------------
// Layout: the reference's sender loop (scatterGCN, gcn_ops.cpp:237-257) over the plan's send lists.  Pack: one kernel over the
// layout's message table.  Deliver: headers parsed and checked on the host, the records through the fixed staging area, one
// unpack kernel per staging slot on the comm stream.  Finish: the round's counters against the ghost count, next round.
uint32_t tensor_layer(dory_ctx *c, const Tensor *t) {
    for (uint32_t l = 0; l < c->tensors.size(); ++l)
        for (auto &kv : c->tensors[l])
            if (&kv.second == t) return l;
    return 0xFFFFFFFFu;
}
inline uint32_t ghost_count(const dory_ctx *c, int dir) { return c->adj[dir == DORY_FORWARD ? ADJ_IN : ADJ_OUT].ghosts; }

void scatter_drop_layouts(dory_ctx *c, int dir /* -1: all */) {
    auto &L = c->scatter.layouts;
    for (size_t i = L.size(); i-- > 0;)
        if (dir < 0 || L[i].dir == dir) {
            if (L[i].d_msgs) (void)hipFree(L[i].d_msgs);
            L.erase(L.begin() + (long)i);
        }
}

// the messages of the exchange of `cols`-wide rows with the plan of `dir` (kept: the same exchange asks again every epoch);
// on_device: with its table uploaded for the pack kernel
int scatter_layout(dory_ctx *c, const char *who, int dir, uint32_t cols, uint64_t max_msg, bool on_device, ScatterLayout **out) {
    const HaloPlan &p = c->plan[dir];
    if (!p.set) return fail(c, DORY_ERR_ARG, "%s: no plan", who);
    if (max_msg > 0xFFFFFFFFull) return fail(c, DORY_ERR_ARG, "%s: max_msg_bytes %llu is not below 2^32", who, (unsigned long long)max_msg);
    if (cols == 0 || cols > scatter_msgs_max_cols())
        return fail(c, DORY_ERR_ARG, "%s: rows of %u floats (scatter messages carry 1 .. %u)", who, cols, scatter_msgs_max_cols());
    if (max_msg == 0) max_msg = DORY_WIRE_MAX_MSG_SIZE;
    ScatterLayout *L = nullptr;
    for (auto &l : c->scatter.layouts)
        if (l.dir == dir && l.cols == cols && l.max_msg == max_msg) L = &l;
    if (!L) {
        if (c->scatter.layouts.size() >= 32) scatter_drop_layouts(c, -1);   // (a caller sweeping message sizes: start over)
        ScatterLayout n;
        n.dir = dir; n.cols = cols; n.max_msg = max_msg;
        const uint32_t batch = dory_wire_scatter_batch(cols, max_msg);
        uint64_t end = 0;
        for (uint32_t q = 0; q < c->numNodes; ++q) {
            if (q == c->nodeId) continue;
            for (uint32_t ib = 0; ib < p.send_counts[q]; ib += batch) {
                dory_scatter_msg m;
                m.peer = q;
                m.first_row = p.send_off[q] + ib;
                m.rows = std::min(batch, p.send_counts[q] - ib);
                m.offset = (end + 15ull) & ~15ull;
                m.bytes = dory_wire_scatter_msg_bytes(m.rows, cols);
                if (m.bytes > 0xFFFFFFFFull) return fail(c, DORY_ERR_ARG, "%s: a message of %llu bytes (below 2^32 only)", who, (unsigned long long)m.bytes);
                end = m.offset + m.bytes;
                n.max_rows = std::max(n.max_rows, m.rows);
                n.msgs.push_back(m);
            }
        }
        n.total_bytes = end;
        c->scatter.layouts.push_back(std::move(n));
        L = &c->scatter.layouts.back();
    }
    if (on_device && !L->d_msgs && !L->msgs.empty()) {
        int rc = upload_array(c, &L->d_msgs, L->msgs.data(), L->msgs.size());
        if (rc) return rc;
    }
    *out = L;
    return DORY_OK;
}

// option halo_direct_recv: ghost slot k is stored at the row the plan's wire order gives it
int scatter_slot_rows(dory_ctx *c, int dir) {
    ScatterState &S = c->scatter;
    const HaloPlan &p = c->plan[dir];
    if (S.d_slot_row[dir]) (void)hipFree(S.d_slot_row[dir]);
    S.d_slot_row[dir] = nullptr;
    if (!S.ids || !p.set || !p.direct) return DORY_OK;
    std::vector<uint32_t> inv(p.recv_total);
    for (uint32_t r = 0; r < p.recv_total; ++r) inv[p.order[r]] = r;
    return upload_array(c, &S.d_slot_row[dir], inv.data(), inv.size());
}

int scatter_pack(dory_ctx *c, const char *who, int dir, const Tensor *src, uint32_t hdr_layer, uint64_t max_msg, void *dev_buf,
                 hipStream_t s, ScatterLayout **layout) {
    if (!c->scatter.ids) return fail(c, DORY_ERR_ARG, "%s: dory_halo_wire_ids first (the records carry global vertex ids)", who);
    if ((uintptr_t)dev_buf & 15) return fail(c, DORY_ERR_ARG, "%s: the message buffer must be 16-byte aligned", who);
    ScatterLayout *L;
    int rc = scatter_layout(c, who, dir, src->cols, max_msg, true, &L);
    if (rc) return rc;
    if (layout) *layout = L;
    if (L->msgs.empty()) return DORY_OK;
    if (!dev_buf) return fail(c, DORY_ERR_ARG, "%s: no buffer", who);
    const HaloPlan &p = c->plan[dir];
    HIPCK(c, launch_scatter_msgs_pack(dev_buf, src->d, src->ld, src->cols, p.d_send_lvids, c->scatter.d_l2g, L->d_msgs, (uint32_t)L->msgs.size(),
                                      L->max_rows, c->nodeId, hdr_layer, (uint32_t)dir, s));
    if (!c->capturing) {
        c->halo_rows_packed += p.send_total;
        c->halo_floats_packed += (uint64_t)p.send_total * src->cols;
    }
    return DORY_OK;
}

// the ghost tensor a message names by (layer, dir), as ghostReceiverGCN / ghostReceiverGAT pick it (gcn_ops.cpp:293-302,
// gat_ops.cpp:366-375), or `name` at the header's layer
Tensor *scatter_ghost_of(dory_ctx *c, const char *name, uint32_t layer, uint32_t dir) {
    if (layer >= c->tensors.size()) return nullptr;
    if (name) return find(c, layer, name);
    if (c->gnn == DORY_GCN) return find(c, layer, dir == DORY_FORWARD ? "fg" : "bg");
    return find(c, layer, dir == DORY_FORWARD ? "fg_z" : "bg_d");
}

int scatter_deliver(dory_ctx *c, const char *name, const void *const *msgs, const uint64_t *bytes, uint32_t n, bool in_cb) {
    const char *who = "scatter_msgs_deliver";
    ScatterState &S = c->scatter;
    if (!msgs || !bytes || n == 0) return fail(c, DORY_ERR_ARG, "%s: at least one message", who);
    if (!S.ids) return fail(c, DORY_ERR_ARG, "%s: dory_halo_wire_ids first", who);
    struct Parsed { Tensor *ghost; uint32_t dir, count, layer; const uint8_t *rec; };
    std::vector<Parsed> P(n);
    // everything is checked before anything is enqueued
    for (uint32_t i = 0; i < n; ++i) {
        if (!msgs[i]) return fail(c, DORY_ERR_ARG, "%s: message %u is null", who, i);
        if (bytes[i] < DORY_WIRE_SCATTER_HDR_SIZE)
            return fail(c, DORY_ERR_ARG, "%s: message %u is truncated: %llu bytes, the header alone has %u", who, i, (unsigned long long)bytes[i], DORY_WIRE_SCATTER_HDR_SIZE);
        const uint8_t *m = static_cast<const uint8_t *>(msgs[i]);
        uint32_t recv = 0, snd = 0, cnt = 0, fd = 0, lay = 0, dr = 0;
        if (dory_wire_parse_scatter_header(m, bytes[i], &recv, &snd, &cnt, &fd, &lay, &dr)) {
            dory_wire_parse_fields_header(m + DORY_WIRE_NODE_ID_DIGITS, &snd, &cnt, &fd, &lay, &dr);
            const uint64_t want = dory_wire_scatter_msg_bytes(cnt, fd);
            if (want != bytes[i])
                return fail(c, DORY_ERR_ARG, "%s: message %u is truncated or malformed: %llu bytes, count %u x featDim %u make %llu", who, i,
                            (unsigned long long)bytes[i], cnt, fd, (unsigned long long)want);
            return fail(c, DORY_ERR_ARG, "%s: message %u: the receiver field is not eight characters of %%8X", who, i);
        }
        if (recv != c->nodeId) return fail(c, DORY_ERR_ARG, "%s: message %u: receiver %u is not this rank (%u)", who, i, recv, c->nodeId);
        if (dr > 1u) return fail(c, DORY_ERR_ARG, "%s: message %u: dir %u is neither forward (0) nor backward (1)", who, i, dr);
        Tensor *ghost;
        if (in_cb && !name) {
            if (lay != S.cb_layer || (int)dr != S.cb_dir)
                return fail(c, DORY_ERR_ARG, "%s: message %u: layer %u dir %u is not the exchange in progress (layer %u dir %d)", who, i, lay, dr, S.cb_layer, S.cb_dir);
            ghost = S.cb_ghost;
        } else {
            if (lay >= c->tensors.size()) return fail(c, DORY_ERR_ARG, "%s: message %u: layer %u out of range", who, i, lay);
            ghost = scatter_ghost_of(c, name, lay, dr);
            if (!ghost) return fail(c, DORY_ERR_ARG, "%s: message %u: layer %u out of range (no ghost tensor '%s' of dir %u there)", who, i, lay,
                                    name ? name : (c->gnn == DORY_GCN ? (dr ? "bg" : "fg") : (dr ? "bg_d" : "fg_z")), dr);
        }
        if (ghost->rows != ghost_count(c, (int)dr) || ghost->rows != S.gvids[dr].size())
            return fail(c, DORY_ERR_ARG, "%s: message %u: the tensor is not a ghost tensor of dir %u", who, i, dr);
        if (fd != ghost->cols) return fail(c, DORY_ERR_ARG, "%s: message %u: featDim %u is not the tensor's cols %u", who, i, fd, ghost->cols);
        if (!c->plan[dr].set) return fail(c, DORY_ERR_ARG, "%s: no plan", who);
        if (fd > scatter_msgs_max_cols() || 4ull * (1ull + fd) > S.stage_bytes)
            return fail(c, DORY_ERR_ARG, "%s: message %u: a record of %u floats does not fit the staging area", who, i, fd);
        P[i] = {ghost, dr, cnt, lay, m + DORY_WIRE_SCATTER_HDR_SIZE};
    }
    for (const Parsed &q : P) {   // what halo_tensors and dory_halo_exchange drop when these ghost rows change
        if (q.ghost == find(c, 0, "fg")) c->ah0_valid = false;
        if (q.ghost == find(c, q.layer, "fg_z") && q.layer < c->gat_nsum_valid.size()) c->gat_nsum_valid[q.layer] = 0;
        ghost_wrote_fp32(q.ghost);   // (dory_halo_bf16_ghosts: records are fp32; a round writes every ghost row)
    }
    std::unique_ptr<Timed> t;
    if (!in_cb) {   // (inside an exchange the comm stream waits already, and the exchange times itself)
        HIPCK(c, hipEventRecord(c->ev_a, c->compute));
        HIPCK(c, hipStreamWaitEvent(c->comm, c->ev_a, 0));
        t.reset(new Timed(c, "halo", c->comm));
    }
    int slot = 0;
    size_t fill = 0;
    const Parsed *cur = nullptr;
    auto flush = [&]() -> int {
        if (!fill) return DORY_OK;
        const uint32_t d = cur->dir, recb = 4u * (1u + cur->ghost->cols);
        HIPCK(c, hipMemcpyAsync(S.d_stage[slot], S.h_stage[slot], fill, hipMemcpyHostToDevice, c->comm));
        HIPCK(c, launch_scatter_msgs_unpack(cur->ghost->d, cur->ghost->ld, cur->ghost->cols, S.d_stage[slot], (uint32_t)(fill / recb), S.d_gvids[d],
                                            (uint32_t)S.gvids[d].size(), S.d_slot_row[d], S.d_stamp[d], S.round[d], S.d_counts[d], c->comm));
        HIPCK(c, hipEventRecord(S.ev_stage[slot], c->comm));
        S.stage_used[slot] = true;
        S.next_slot = slot ^ 1;
        fill = 0;
        return DORY_OK;
    };
    for (const Parsed &q : P) {
        if (cur && (cur->ghost != q.ghost || cur->dir != q.dir)) { int rc = flush(); if (rc) return rc; }
        cur = &q;
        const size_t recb = 4u * (size_t)(1u + q.ghost->cols);
        uint32_t left = q.count;
        const uint8_t *rec = q.rec;
        while (left) {
            if (!fill) {   // a fresh slot: free once the unpack that read it last has run
                slot = S.next_slot;
                if (S.stage_used[slot]) HIPCK(c, hipEventSynchronize(S.ev_stage[slot]));
            }
            const uint32_t take = (uint32_t)std::min<size_t>(left, (S.stage_bytes - fill) / recb);
            std::memcpy(S.h_stage[slot] + fill, rec, take * recb);
            fill += take * recb;
            rec += take * recb;
            left -= take;
            if (S.stage_bytes - fill < recb) { int rc = flush(); if (rc) return rc; }
        }
    }
    return flush();
}

int scatter_finish(dory_ctx *c, int dir, uint32_t *rows, uint32_t *unknown, uint32_t *duplicate) {
    ScatterState &S = c->scatter;
    uint32_t h[3] = {0, 0, 0};
    HIPCK(c, hipMemcpyAsync(h, S.d_counts[dir], sizeof(h), hipMemcpyDeviceToHost, c->comm));
    HIPCK(c, hipMemsetAsync(S.d_counts[dir], 0, sizeof(h), c->comm));
    HIPCK(c, hipStreamSynchronize(c->comm));
    if (++S.round[dir] == 0) S.round[dir] = 1;   // (the stamps start at 0: never a round's number)
    if (rows) *rows = h[0];
    if (unknown) *unknown = h[1];
    if (duplicate) *duplicate = h[2];
    const uint32_t G = (uint32_t)S.gvids[dir].size();
    if (h[0] != G || h[1] || h[2])
        return fail(c, DORY_ERR_COMM, "scatter_msgs_finish: %u of %u ghost rows of dir %d written, %u records with unknown ids, %u duplicates", h[0], G, dir, h[1], h[2]);
    return DORY_OK;
}

int scatter_send_buffers(dory_ctx *c, size_t bytes) {
    ScatterState &S = c->scatter;
    if (bytes <= S.send_cap) return DORY_OK;
    HIPCK(c, hipDeviceSynchronize());
    if (S.d_send) (void)hipFree(S.d_send);
    if (S.h_send) (void)hipHostFree(S.h_send);
    S.d_send = S.h_send = nullptr; S.send_cap = 0;
    HIPCK(c, hipMalloc((void **)&S.d_send, bytes));
    HIPCK(c, hipHostMalloc((void **)&S.h_send, bytes, hipHostMallocDefault));
    S.send_cap = bytes;
    return DORY_OK;
}

// the scatter transport's arm of an exchange (the comm stream waits for the producer of `src` already): pack the messages, copy
// them to pinned host memory, let the caller's function send them and deliver what arrived, finish the round
int exchange_scatter(dory_ctx *c, int dir, Tensor *src, Tensor *ghost) {
    ScatterState &S = c->scatter;
    if (src->cols != ghost->cols) return fail(c, DORY_ERR_ARG, "halo_exchange: widths of source (%u) and ghost tensor (%u) differ", src->cols, ghost->cols);
    if (!S.ids) return fail(c, DORY_ERR_ARG, "halo_exchange: the scatter transport needs dory_halo_wire_ids");
    const uint32_t hdr_layer = tensor_layer(c, ghost);
    ScatterLayout *L;
    int rc = scatter_layout(c, "halo_exchange", dir, src->cols, S.max_msg, true, &L);
    if (rc) return rc;
    if ((rc = scatter_send_buffers(c, (size_t)L->total_bytes))) return rc;
    if ((rc = scatter_pack(c, "halo_exchange", dir, src, hdr_layer, S.max_msg, S.d_send, c->comm, nullptr))) return rc;
    if (L->total_bytes) HIPCK(c, hipMemcpyAsync(S.h_send, S.d_send, (size_t)L->total_bytes, hipMemcpyDeviceToHost, c->comm));
    HIPCK(c, hipStreamSynchronize(c->comm));
    S.cb_thread = std::this_thread::get_id();
    S.cb_ghost = ghost; S.cb_layer = hdr_layer; S.cb_dir = dir;
    S.in_cb.store(true, std::memory_order_release);
    const int cb = S.fn(c->tx_user, c, S.h_send, L->msgs.data(), (uint32_t)L->msgs.size());
    S.in_cb.store(false, std::memory_order_release);
    S.cb_ghost = nullptr;
    const std::string cb_err = c->err;   // (a refusal of dory_scatter_msgs_deliver inside the callback: keep its text)
    rc = scatter_finish(c, dir, nullptr, nullptr, nullptr);
    if (cb) return fail(c, DORY_ERR_COMM, "halo_exchange: scatter transport exchange failed (%d)%s%s", cb, cb_err.empty() ? "" : ": ", cb_err.c_str());
    return rc;
}

// ---------------------------------------------------------------------------------------
// In-process device transport (dory_comm_init_local): P contexts of one process on one device are each other's peers.
// One exchange = pack on the sender's comm stream -> hipMemcpyAsync device -> device into every peer's receive buffer on
// the SENDER's comm stream -> event "sent"; the receiver's comm stream waits for its peers' "sent" events, unpacks, records
// "consumed" (its receive buffer is free again) and the event the compute stream waits for.  Same stream / event structure
// as the RCCL arm, no host synchronisation with the device anywhere: what the overlapped schedule of Engine::scatterGCN +
// ghostReceiver (gcn_ops.cpp:204-282 send, :284-362 receive) looks like when copies really run beside the aggregation.
// A stream never waits for an event that is not recorded yet (hipStreamWaitEvent on an unrecorded event is a no-op, and a
// device-side wait for work a host thread has still to enqueue deadlocks with any device-wide synchronisation, e.g. a
// hipFree in a lazy allocation): every event has a progress counter its owner bumps AFTER recording, and a context reads
// the peer's counter BEFORE it makes its stream wait.  That read may block the calling host thread until the peer's host
// thread has got there (bounded: option local_timeout_ms) -- so the ranks must be driven by one host thread each, or stage
// by stage (all ranks' scatter before any rank's next gather), exactly as real ranks are.
constexpr uint32_t LOCAL_MAX_RANKS = 16;

int local_wait_posted(dory_ctx *c, const std::atomic<uint64_t> &ctr, uint64_t want, uint32_t peer, const char *what) {
    if (ctr.load(std::memory_order_acquire) >= want) return DORY_OK;
    const int64_t lim = c->opt[OPT_LOCAL_TIMEOUT_MS] > 0 ? c->opt[OPT_LOCAL_TIMEOUT_MS] : 30000;
    const auto deadline = std::chrono::steady_clock::now() + std::chrono::milliseconds(lim);
    uint32_t spins = 0;
    while (ctr.load(std::memory_order_acquire) < want) {
        if (++spins < 2000) std::this_thread::yield();
        else std::this_thread::sleep_for(std::chrono::microseconds(50));
        if ((spins & 255u) == 0 && std::chrono::steady_clock::now() > deadline)
            return fail(c, DORY_ERR_COMM, "local transport: rank %u did not reach %s %llu within %lld ms (every rank needs its own host thread, or "
                        "stage-by-stage driving)", peer, what, (unsigned long long)want, (long long)lim);
    }
    return DORY_OK;
}

// Option halo_direct_recv, first half: the RECEIVER pulls, so a sender's part is pack and "sent".  What a peer's "consumed" of
// exchange s - 1 now frees is MY send buffer (it has copied its rows out of it): the same counter and event, waited for in
// the same place as the push form waits for them -- the first half of exchange s, before anything is enqueued -- by the
// ranks that sent to that peer in exchange s - 1 (the push form: that send to it in exchange s; the same ranks wherever both
// directions' plans name the same peers).  No host-side wait is added.
int local_pull_send(dory_ctx *c, int dir, const HaloPlan &p, Tensor *src, RowWire wire, uint64_t s) {
    LocalGroup &grp = *c->local;
    for (uint32_t q = 0; q < c->numNodes && s > 1; ++q) {
        if (q == c->nodeId || q >= c->local_sent_to.size() || !c->local_sent_to[q]) continue;
        dory_ctx *Q = grp.ctx[q];
        if (!Q) return fail(c, DORY_ERR_COMM, "local transport: rank %u has been destroyed", q);
        int rc = local_wait_posted(c, Q->posted_cons, s - 1, q, "the receive of exchange");
        if (rc) return rc;
        HIPCK(c, hipStreamWaitEvent(c->comm, Q->ev_cons[(s - 1) & 1], 0));
    }
    { int rc = send_rows(c, src, dir, wire, p, c->comm, false); if (rc) return rc; }   // (the peers read my send buffer on their own streams: never fused)
    c->local_sent_to.assign(c->numNodes, 0);
    for (uint32_t q = 0; q < c->numNodes; ++q) c->local_sent_to[q] = q != c->nodeId && p.send_counts[q] != 0;
    return DORY_OK;
}

// first half of an exchange: pack, push my rows into every peer's receive buffer, "sent"; the second half
// (local_exchange_finish, below) at once, or with `deferred` when wait_halo() is next called
int exchange_local(dory_ctx *c, int dir, Tensor *src, Tensor *ghost, RowWire wire, bool deferred, const RowPair *pair) {
    HaloPlan &p = c->plan[dir];
    LocalGroup &grp = *c->local;
    const size_t rb = wire.row_bytes();
    if (c->local_pending.on) {   // (not reached: every consumer and every exchange calls wait_halo first)
        int rc = local_exchange_finish(c);
        if (rc) return rc;
    }
    const uint64_t s = ++c->local_seq;
    dory_ctx::LocalPending &lp = c->local_pending;
    timed_open(c, "halo", c->comm, &lp.t_halo_b);
    timed_open(c, deferred ? "halo_deferred" : "halo_waited", c->comm, &lp.t_kind_b);
    if (p.direct) { int rc = local_pull_send(c, dir, p, src, wire, s); if (rc) return rc; }
    else { int rc = send_rows(c, src, dir, wire, p, c->comm, true, pair); if (rc) return rc; }
    for (uint32_t q = 0; q < c->numNodes && !p.direct; ++q) {
        if (q == c->nodeId || !p.send_counts[q]) continue;
        dory_ctx *Q = grp.ctx[q];
        if (!Q) return fail(c, DORY_ERR_COMM, "local transport: rank %u has been destroyed", q);
        const HaloPlan &pq = Q->plan[dir];
        if (!pq.set || pq.recv_counts.size() != c->numNodes || pq.recv_counts[c->nodeId] != p.send_counts[q])
            return fail(c, DORY_ERR_COMM, "local transport: rank %u expects %u rows from rank %u, which sends %u", q,
                        pq.set && pq.recv_counts.size() == c->numNodes ? pq.recv_counts[c->nodeId] : 0u, c->nodeId, p.send_counts[q]);
        if ((size_t)pq.recv_total * rb > Q->recv_cap)
            return fail(c, DORY_ERR_COMM, "local transport: receive buffer of rank %u too small for rows of %zu bytes", q, rb);
        if (s > 1) {   // its receive buffer must have been unpacked (exchange s - 1)
            int rc = local_wait_posted(c, Q->posted_cons, s - 1, q, "the unpack of exchange");
            if (rc) return rc;
            HIPCK(c, hipStreamWaitEvent(c->comm, Q->ev_cons[(s - 1) & 1], 0));
        }
        HIPCK(c, hipMemcpyAsync((char *)Q->recv_buf + (size_t)pq.recv_off[c->nodeId] * rb, (const char *)c->send_buf + (size_t)p.send_off[q] * rb,
                                (size_t)p.send_counts[q] * rb, hipMemcpyDeviceToDevice, c->comm));
    }
    HIPCK(c, hipEventRecord(c->ev_sent[s & 1], c->comm));
    c->posted_sent.store(s, std::memory_order_release);
    lp.on = true;
    lp.dir = dir;
    lp.keep = keeps_bf16(c, wire, ghost);
    lp.ghost = lp.keep ? reinterpret_cast<char *>(ghost->twin) : reinterpret_cast<char *>(ghost->d);
    lp.ghost_ld = ghost->ld;
    lp.ghost2 = pair ? pair->ghost2->d : nullptr;
    lp.ghost2_ld = pair ? pair->ghost2->ld : 0;
    lp.wire = wire;
    lp.direct = lands_directly(p, wire, ghost->ld, lp.keep);
    lp.widen_to = lp.keep && ghost->raw_handed ? ghost->d : nullptr;
    lp.ghost_rows = ghost->rows;
    { int rc = ghost_rows_landed(c, ghost, lp.keep, lp.direct, c->comm, false, dir, pair != nullptr); if (rc) return rc; }   // (every reader calls wait_halo first: the second half)
    if (deferred) {
        c->halo_pending = true;      // wait_halo(): local_exchange_finish, then the compute stream waits for ev_b
        return DORY_OK;
    }
    int rc = local_exchange_finish(c);
    if (rc) return rc;
    HIPCK(c, hipStreamWaitEvent(c->compute, c->ev_b, 0));
    return DORY_OK;
}

// ---- the other two arms: the packed rows in c->send_buf travel, the peers' rows arrive in `recv` (comm stream) ----------
// host transport: the bytes travel through the caller (c->tx_recv is still being read when this returns)
// (w: the floats of a row on the wire, RowWire::row_bytes() / 4 -- bf16 rows travel as w / 2 floats' worth of bytes)
int exchange_host(dory_ctx *c, const HaloPlan &p, uint32_t w, float *recv /* c->recv_buf, or the ghost tensor (halo_direct_recv) */) {
    const size_t sb = (size_t)p.send_total * w * sizeof(float), rb = (size_t)p.recv_total * w * sizeof(float);
    c->tx_send.resize((size_t)p.send_total * w);
    c->tx_recv.resize((size_t)p.recv_total * w);
    if (sb) HIPCK(c, hipMemcpyAsync(c->tx_send.data(), c->send_buf, sb, hipMemcpyDeviceToHost, c->comm));
    HIPCK(c, hipStreamSynchronize(c->comm));
    std::vector<uint64_t> sc(c->numNodes), so(c->numNodes), rc_(c->numNodes), ro(c->numNodes);
    for (uint32_t peer = 0; peer < c->numNodes; ++peer) {
        sc[peer] = (uint64_t)p.send_counts[peer] * w; so[peer] = (uint64_t)p.send_off[peer] * w;
        rc_[peer] = (uint64_t)p.recv_counts[peer] * w; ro[peer] = (uint64_t)p.recv_off[peer] * w;
    }
    if (c->tx_a2a(c->tx_user, c->tx_send.data(), sc.data(), so.data(), c->tx_recv.data(), rc_.data(), ro.data(), c->numNodes))
        return fail(c, DORY_ERR_COMM, "halo_exchange: host transport alltoallv failed");
    if (rb) HIPCK(c, hipMemcpyAsync(recv, c->tx_recv.data(), rb, hipMemcpyHostToDevice, c->comm));
    return DORY_OK;
}
// RCCL: grouped ncclSend / ncclRecv
int exchange_rccl(dory_ctx *c, const HaloPlan &p, uint32_t w, float *recv /* as exchange_host's */) {
    ncclComm_t comm = (ncclComm_t)c->nccl;
    NCCLCK(c, ncclGroupStart());
    for (uint32_t peer = 0; peer < c->numNodes; ++peer) {
        if (peer == c->nodeId) continue;
        if (p.send_counts[peer])
            NCCLCK(c, ncclSend(c->send_buf + (size_t)p.send_off[peer] * w, (size_t)p.send_counts[peer] * w,
                               ncclFloat, (int)peer, comm, c->comm));
        if (p.recv_counts[peer])
            NCCLCK(c, ncclRecv(recv + (size_t)p.recv_off[peer] * w, (size_t)p.recv_counts[peer] * w,
                               ncclFloat, (int)peer, comm, c->comm));
    }
    NCCLCK(c, ncclGroupEnd());
    return DORY_OK;
}

// ---- all-reduce -----------------------------------------------------------------------------------------------------------
struct PeerPtrs { const float *p[LOCAL_MAX_RANKS]; };
__global__ __launch_bounds__(256) void local_sum_kernel(PeerPtrs pp, uint32_t P, uint64_t n, float *out) {
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x) {
        float sum = 0.f;
        for (uint32_t q = 0; q < P; ++q) sum += pp.p[q][i];      // rank order on every rank: identical bits everywhere
        out[i] = sum;
    }
}

// sum of n floats over the group into gd: every rank adds the P buffers in rank order (identical bits on every rank).
// peer_buf(Q) = that buffer of rank Q (mine included), or null after recording why rank Q has none of this shape
template <typename PeerBuf>
int local_allreduce(dory_ctx *c, float *gd, uint64_t n, PeerBuf peer_buf) {
    LocalGroup &grp = *c->local;
    const uint32_t P = c->numNodes;
    if (n * sizeof(float) > c->ar_tmp_cap) return fail(c, DORY_ERR_COMM, "local transport: gradient staging buffer too small (preallocate before dory_comm_init_local)");
    const uint64_t t = ++c->local_ar_seq;
    HIPCK(c, hipEventRecord(c->ev_gready[t & 1], c->compute));
    c->posted_g.store(t, std::memory_order_release);
    PeerPtrs pp{};
    for (uint32_t q = 0; q < P; ++q) {
        dory_ctx *Q = q == c->nodeId ? c : grp.ctx[q];
        if (!Q) return fail(c, DORY_ERR_COMM, "local transport: rank %u has been destroyed", q);
        if (q != c->nodeId) {
            int rc = local_wait_posted(c, Q->posted_g, t, q, "gradient sum");
            if (rc) return rc;
            HIPCK(c, hipStreamWaitEvent(c->compute, Q->ev_gready[t & 1], 0));
        }
        if (!(pp.p[q] = peer_buf(Q))) return DORY_ERR_COMM;
    }
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(1024, (n + 255) / 256);
    hipLaunchKernelGGL(local_sum_kernel, dim3(blocks), dim3(256), 0, c->compute, pp, P, n, c->ar_tmp);
    HIPCK(c, hipGetLastError());
    HIPCK(c, hipEventRecord(c->ev_gdone[t & 1], c->compute));
    c->posted_gdone.store(t, std::memory_order_release);
    for (uint32_t q = 0; q < P; ++q) {     // nobody reads my gradient any more: the sum may replace it
        if (q == c->nodeId) continue;
        dory_ctx *Q = grp.ctx[q];
        int rc = local_wait_posted(c, Q->posted_gdone, t, q, "the end of gradient sum");
        if (rc) return rc;
        HIPCK(c, hipStreamWaitEvent(c->compute, Q->ev_gdone[t & 1], 0));
    }
    HIPCK(c, hipMemcpyAsync(gd, c->ar_tmp, n * sizeof(float), hipMemcpyDeviceToDevice, c->compute));
    return DORY_OK;
}

// Sum of n floats at device pointer `buf` over all ranks, in place, on the compute stream: the sum of per-partition updates
// (WeightTensor::localUpdate/ghostUpdate, src/weight-server/weighttensor.cpp:131-166) as one collective.  peer_buf: see
// local_allreduce (the in-process transport reads the peers' buffers itself).
template <typename PeerBuf>
int allreduce_sum(dory_ctx *c, const char *who, float *buf, uint64_t n, PeerBuf peer_buf) {
    switch (transport_of(c)) {
    case Transport::Host:
    case Transport::Scatter:   // (the gradient sum is the host transport arm's)
        c->tx_send.resize(n);
        HIPCK(c, hipMemcpyAsync(c->tx_send.data(), buf, n * sizeof(float), hipMemcpyDeviceToHost, c->compute));
        HIPCK(c, hipStreamSynchronize(c->compute));
        if (c->tx_ar(c->tx_user, c->tx_send.data(), n)) return fail(c, DORY_ERR_COMM, "%s: host transport allreduce failed", who);
        HIPCK(c, hipMemcpyAsync(buf, c->tx_send.data(), n * sizeof(float), hipMemcpyHostToDevice, c->compute));
        HIPCK(c, hipStreamSynchronize(c->compute));
        return DORY_OK;
    case Transport::Local:
        return local_allreduce(c, buf, n, peer_buf);
    case Transport::Rccl:
        NCCLCK(c, ncclAllReduce(buf, buf, n, ncclFloat, ncclSum, (ncclComm_t)c->nccl, c->compute));
        return DORY_OK;
    case Transport::None:   // (reached from dory_train_stat_global only: dory_weight_update refuses before its "allreduce" interval opens)
        break;
    }
    return fail(c, DORY_ERR_COMM, "%s: dory_comm_init not called", who);
}

// AdamOptimizer::nextIteration (src/weight-server/AdamOptimizer.cpp:29-34): the step size of iteration `epochs`
float adam_lr_t(const dory_ctx *c, unsigned epochs) {
    const float b1p = (float)std::pow((double)0.9f, (double)epochs);
    const float b2p = (float)std::pow((double)0.999f, (double)epochs);
    return (float)(c->adam.lr * (std::sqrt((double)(1 - b2p))) / (1 - b1p));
}

}  // namespace

namespace dory {

// second half of an exchange: the peers' rows have been sent (their "sent" events) -> unpack -> "consumed" + ev_b
int local_exchange_finish(dory_ctx *c) {
    dory_ctx::LocalPending &lp = c->local_pending;
    if (!lp.on) return DORY_OK;
    HaloPlan &p = c->plan[lp.dir];
    const uint64_t s = c->local_seq;
    LocalGroup &grp = *c->local;
    for (uint32_t q = 0; q < c->numNodes; ++q) {
        // only the peers that send me rows: a peer that sends me nothing does not wait for my receive buffer either, may be
        // exchanges ahead, and its event ring (two deep) would by then hold a LATER exchange's record -- one that can depend
        // on work queued behind this very wait
        if (q == c->nodeId || !p.recv_counts[q]) continue;
        dory_ctx *Q = grp.ctx[q];
        if (!Q) return fail(c, DORY_ERR_COMM, "local transport: rank %u has been destroyed", q);
        int rc = local_wait_posted(c, Q->posted_sent, s, q, "exchange");
        if (rc) return rc;
        HIPCK(c, hipStreamWaitEvent(c->comm, Q->ev_sent[s & 1], 0));
    }
    lp.on = false;     // (a peer that has not arrived leaves the second half pending: the caller may try again)
    if (p.direct) {   // option halo_direct_recv: I pull every peer's segment out of its send buffer -- into the ghost tensor (the
        // wire's width is its ld), or into my receive buffer for the unpack (exact rows narrower than ld)
        const size_t rb = lp.wire.row_bytes();
        char *dst = lp.direct ? lp.ghost : reinterpret_cast<char *>(c->recv_buf);
        for (uint32_t q = 0; q < c->numNodes; ++q) {
            if (q == c->nodeId || !p.recv_counts[q]) continue;
            const dory_ctx *Q = grp.ctx[q];
            const HaloPlan &pq = Q->plan[lp.dir];
            if (!pq.set || pq.send_counts.size() != c->numNodes || pq.send_counts[c->nodeId] != p.recv_counts[q])
                return fail(c, DORY_ERR_COMM, "local transport: rank %u expects %u rows from rank %u, which sends %u", c->nodeId, p.recv_counts[q], q,
                            pq.set && pq.send_counts.size() == c->numNodes ? pq.send_counts[c->nodeId] : 0u);
            if ((size_t)pq.send_total * rb > Q->send_cap)
                return fail(c, DORY_ERR_COMM, "local transport: send buffer of rank %u too small for rows of %zu bytes", q, rb);
            HIPCK(c, hipMemcpyAsync(dst + (size_t)p.recv_off[q] * rb, (const char *)Q->send_buf + (size_t)pq.send_off[c->nodeId] * rb,
                                    (size_t)p.recv_counts[q] * rb, hipMemcpyDeviceToDevice, c->comm));
        }
    }
    if (!lp.direct) {
        int rc = unpack_rows(c, lp.keep ? nullptr : reinterpret_cast<float *>(lp.ghost), lp.ghost_ld, lp.wire, c->recv_buf, p, c->comm,
                             lp.keep ? reinterpret_cast<uint16_t *>(lp.ghost) : nullptr, lp.ghost2, lp.ghost2_ld);
        if (rc) return rc;
    }
    // (dory_halo_bf16_ghosts, the tensor's raw pointer is out: its fp32 rows follow the twin at once)
    if (lp.widen_to) HIPCK(c, launch_widen_rows_bf16(lp.widen_to, reinterpret_cast<const uint16_t *>(lp.ghost), lp.ghost_rows * lp.ghost_ld, c->comm));
    HIPCK(c, hipEventRecord(c->ev_cons[s & 1], c->comm));
    c->posted_cons.store(s, std::memory_order_release);
    if (lp.t_kind_b) (void)hipEventRecord(lp.t_kind_b, c->comm);
    if (lp.t_halo_b) (void)hipEventRecord(lp.t_halo_b, c->comm);
    lp.t_kind_b = lp.t_halo_b = nullptr;
    HIPCK(c, hipEventRecord(c->ev_b, c->comm));
    return DORY_OK;
}

// Ghost rows of the last halo exchange land on the comm stream; with "halo_overlap" the
// compute stream is only made to wait for them (event ev_b) by the first consumer.
int wait_halo(dory_ctx *c) {
    if (c->halo_pending) {
        if (c->local_pending.on) {   // in-process device transport: the peers' rows, unpack, ev_b
            int rc = local_exchange_finish(c);
            if (rc) return rc;
        }
        HIPCK(c, hipStreamWaitEvent(c->compute, c->ev_b, 0));
        c->halo_pending = false;
        if (c->gatmh_scores_pending >= 0) return gatmh_ghost_scores_flush(c);   // (dory_gatmh_row_gather_overlap: left by dory_apply_edge)
    }
    return DORY_OK;
}

// One all-to-all-v of rows: src rows listed in plan[dir] -> the peers' ghost tensors.  pack -> the transport's arm ->
// unpack on the comm stream, ordered after the compute stream's work so far; the compute stream waits for the ghosts
// at once (defer == false) or when wait_halo() is next called (halo_overlap).
// `pair` (dory_gatmh_bwd_merged_exchange; gatmh_bwd_exchange has checked transport and plan): merged rows [src | pair->src2] into
// ghost and pair->ghost2 -- the same arms, a row of w + w2 floats.
int exchange_rows(dory_ctx *c, int dir, Tensor *src, Tensor *ghost, bool defer, const RowPair *pair, bool follows_rule) {
    HaloPlan &p = c->plan[dir];
    if (!p.set) return fail(c, DORY_ERR_ARG, "halo_exchange: no plan");
    const Transport tr = transport_of(c);
    if (tr == Transport::None) return fail(c, DORY_ERR_COMM, "halo_exchange: dory_comm_init not called");
    if (tr == Transport::Rccl && c->nranks != (int)c->numNodes) return fail(c, DORY_ERR_COMM, "halo_exchange: communicator size != num_nodes");
    if (src->ld != ghost->ld) return fail(c, DORY_ERR_ARG, "halo_exchange: row widths of source and ghost tensor differ");
    if (tr == Transport::Scatter) {   // messages of (id, cols floats) records: no row wire, no receive buffer; scheduled as the host arm is
        HIPCK(c, hipEventRecord(c->ev_a, c->compute));
        HIPCK(c, hipStreamWaitEvent(c->comm, c->ev_a, 0));
        const bool deferred = defer && c->opt[OPT_HALO_OVERLAP];
        if (sw_on(c, SW_HALO_FUSED_PACK) && !c->capturing) c->count[CNT_FALLBACK_EXCHANGES]++;   // (messages have another layout: never fused)
        fp32_while_on(c);   // (... and carry fp32)
        {
            Timed t(c, "halo", c->comm);
            Timed td(c, deferred ? "halo_deferred" : "halo_waited", c->comm);
            int rc = exchange_scatter(c, dir, src, ghost);
            if (rc) return rc;
        }
        HIPCK(c, hipEventRecord(c->ev_b, c->comm));
        if (deferred) c->halo_pending = true;
        else HIPCK(c, hipStreamWaitEvent(c->compute, c->ev_b, 0));
        return DORY_OK;
    }
    RowWire wire;
    { int rc = row_wire(c, "halo_exchange", src, ghost, true, nullptr, follows_rule ? dir : -1, &wire); if (rc) return rc; }
    const bool ships16 = wire.bf16;   // (what the rule says of this exchange: the peers of the local transport must say the same)
    if (pair) {
        if (p.direct || (wire.bf16 && c->gnn != DORY_GATMH) || pair->src2->ld != pair->ghost2->ld || pair->src2->cols != pair->ghost2->cols)
            return fail(c, DORY_ERR_ARG, "halo_exchange: merged rows need a plan without halo_direct_recv and two tensors of one shape at either end");
        wire = pair_wire(c, src, pair->src2, ships16);
    }
    const uint32_t w = wire.w;
    const size_t row_b = wire.row_bytes();
    if (tr == Transport::Local) {   // every rank packs and unpacks at one width: checked here, before anything of this exchange is enqueued or counted
        for (uint32_t q = 0; q < c->numNodes; ++q) {
            dory_ctx *Q = q == c->nodeId ? nullptr : c->local->ctx[q];
            if (Q && halo_exact(Q) != wire.exact)
                return fail(c, DORY_ERR_COMM, "local transport: option halo_exact_rows differs: rank %u has %d, rank %u has %d (all ranks must agree)",
                            c->nodeId, (int)wire.exact, q, (int)!wire.exact);
            if (Q && halo_direct(Q) != p.direct)   // (who pushes and who pulls)
                return fail(c, DORY_ERR_COMM, "local transport: option halo_direct_recv differs: rank %u has %d, rank %u has %d (all ranks must agree)",
                            c->nodeId, (int)p.direct, q, (int)!p.direct);
            if (Q && c->gnn == DORY_GATMH && sw_on(Q, SW_GATMH_BF16_GHOSTS) != sw_on(c, SW_GATMH_BF16_GHOSTS))
                return fail(c, DORY_ERR_COMM, "local transport: dory_gatmh_bf16_ghosts differs: rank %u has %d, rank %u has %d (all ranks must agree)",
                            c->nodeId, (int)sw_on(c, SW_GATMH_BF16_GHOSTS), q, (int)sw_on(Q, SW_GATMH_BF16_GHOSTS));
            // what each rank would ship: the switch, the gather mode that drives the rule, and -- under a direct plan (the same on both by
            // now) -- dory_halo_bf16_ghosts, without which such a plan keeps fp32
            const bool q_ships = Q && follows_rule && halo_ships_bf16(Q, dir) && (!p.direct || direct_keeps(Q, ghost->ld));
            if (Q && q_ships != ships16)
                return fail(c, DORY_ERR_COMM, "local transport: dory_halo_bf16_rows differs: rank %u ships %s rows, rank %u %s rows (the switch and the "
                            "gather mode must be the same on all ranks%s%s)", c->nodeId, ships16 ? "bf16" : "fp32", q, ships16 ? "fp32" : "bf16",
                            p.direct ? ", and dory_halo_bf16_ghosts under halo_direct_recv" : "", c->gnn == DORY_GATMH ? ", and dory_gatmh_halo_bf16" : "");
        }
    }
    const bool keep = keeps_bf16(c, wire, ghost);
    const bool direct = lands_directly(p, wire, ghost->ld, keep);
    if (wire.bf16 && p.direct && !keep)   // (not reached: every tensor halo_route names for a model that ships bf16 has a twin while the switch is on)
        return fail(c, DORY_ERR_ARG, "halo_exchange: dory_halo_bf16_ghosts: the ghost tensor has no bf16 twin for a plan made with halo_direct_recv = 1");
    if ((direct || keep) && ghost->rows != p.recv_total)   // (the received rows are written at the tensor's own stride: it must hold exactly them)
        return fail(c, DORY_ERR_ARG, "halo_exchange: ghost tensor of %llu rows for a plan that receives %u", (unsigned long long)ghost->rows, p.recv_total);
    // (option halo_direct_recv: a receive buffer only where dory_halo_plan allocated one -- never inside an epoch)
    const size_t sb = (size_t)p.send_total * row_b, rb = direct ? 0 : (size_t)p.recv_total * row_b;
    if (p.direct && rb > c->recv_cap) return fail(c, DORY_ERR_ARG, NO_RECV_BUF, w, ghost->ld);
    if (tr == Transport::Local && (sb > c->send_cap || rb > c->recv_cap))
        return fail(c, DORY_ERR_COMM, "local transport: exchange buffers too small for %u-float rows (peers hold their addresses: no regrowth)", w);
    // (no growth after dory_halo_plan sized them for the widest layer: only for a tensor uploaded with other dimensions than
    // dory_configure's)
    { int rc = ensure_exchange_buffers(c, sb, rb); if (rc) return rc; }
    // comm stream waits for the producer of `src` on the compute stream
    HIPCK(c, hipEventRecord(c->ev_a, c->compute));
    HIPCK(c, hipStreamWaitEvent(c->comm, c->ev_a, 0));
    const bool deferred = defer && c->opt[OPT_HALO_OVERLAP];
    (direct ? c->halo_direct_recvs : c->halo_staged_recvs) += 1;
    if (tr == Transport::Local) return exchange_local(c, dir, src, ghost, wire, deferred, pair);
    {   // host transport and RCCL: same pack / unpack / events, only the way from send_buf to recv_buf differs
        Timed t(c, "halo", c->comm);
        Timed td(c, deferred ? "halo_deferred" : "halo_waited", c->comm);   // (overlap bookkeeping: abi_internal.hpp)
        int rc = send_rows(c, src, dir, wire, p, c->comm, true, pair);
        // (dory_halo_bf16_ghosts: bf16 rows that land directly land in the twin -- ld / 2 floats' worth of bytes a row)
        float *recv = !direct ? c->recv_buf : keep ? reinterpret_cast<float *>(ghost->twin) : ghost->d;
        const uint32_t wf = (uint32_t)(row_b / sizeof(float));
        if (!rc) rc = tr == Transport::Host ? exchange_host(c, p, wf, recv) : exchange_rccl(c, p, wf, recv);
        if (!rc && !direct)
            rc = unpack_rows(c, ghost->d, ghost->ld, wire, c->recv_buf, p, c->comm, keep ? ghost->twin : nullptr, pair ? pair->ghost2->d : nullptr,
                             pair ? pair->ghost2->ld : 0);
        if (!rc) rc = ghost_rows_landed(c, ghost, keep, direct, c->comm, true, dir, pair != nullptr);
        if (!rc && pair) ghost_wrote_fp32(pair->ghost2);
        if (rc) return rc;
        // the one step of an arm left in the shared body: the host arm's, but it stays behind the unpack, so that the unpack
        // is enqueued before the host blocks for the copy out of tx_recv (which the next exchange reuses)
        if (tr == Transport::Host) HIPCK(c, hipStreamSynchronize(c->comm));
    }
    HIPCK(c, hipEventRecord(c->ev_b, c->comm));
    if (deferred) c->halo_pending = true;
    else HIPCK(c, hipStreamWaitEvent(c->compute, c->ev_b, 0));
    return DORY_OK;
}

// ---- dory_gatmh_bwd_merged_exchange: do -> bg_do and st -> bg_st between the two phases of a whole backward sweep --------------
// the widest merged row any layer of the model ships, padded wire (what dory_halo_plan and the setter size the buffers by)
uint32_t gatmh_merged_row_max(const dory_ctx *c) {
    uint32_t r = 0;
    for (uint32_t l = 0; l < c->L && l < c->heads.size() && l + 1 < c->dims.size(); ++l) {
        const uint32_t K = c->heads[l], zw = l == c->L - 1 ? c->dims[l + 1] * K : c->dims[l + 1];
        r = std::max(r, pad_ld(zw) + 4 * K);
    }
    return r;
}
// the merged exchange is taken: the switch, a whole sweep, a transport that moves dense rows, a plan whose received rows go through
// the receive buffer (halo_direct_recv lands rows in ONE tensor)
static bool gatmh_merged_taken(const dory_ctx *c) {
    if (!sw_on(c, SW_GATMH_BWD_MERGED_EXCHANGE) || c->opt[OPT_GATMH_BWD_PHASE] != 0 || c->numNodes <= 1) return false;
    const Transport tr = transport_of(c);
    return (tr == Transport::Rccl || tr == Transport::Host || tr == Transport::Local) && c->plan[DORY_BACKWARD].set && !c->plan[DORY_BACKWARD].direct;
}
int gatmh_bwd_send_target(dory_ctx *c, const Tensor *dO, const Tensor *st, GatmhSend *sd, bool *send, bool *bf16) {
    const HaloPlan &p = c->plan[DORY_BACKWARD];
    *send = *bf16 = false;
    if (!gatmh_merged_taken(c) || !sw_on(c, SW_HALO_FUSED_PACK) || c->capturing || !p.d_send_map || p.send_map_rows != c->N || dO->rows != c->N) return DORY_OK;
    const bool do16 = gatmh_do_bf16(c, dO);
    const RowWire wire = pair_wire(c, dO, st, do16);
    if ((size_t)p.send_total * wire.row_bytes() > c->send_cap) return DORY_OK;   // (the exchange would regrow the buffer)
    if (transport_of(c) == Transport::Local)   // (its refusal comes from gatmh_bwd_exchange / exchange_rows, before anything is written)
        for (uint32_t q = 0; q < c->numNodes; ++q) {
            const dory_ctx *Q = q == c->nodeId ? nullptr : c->local->ctx[q];
            if (Q && (!sw_on(Q, SW_GATMH_BWD_MERGED_EXCHANGE) || halo_ships_bf16(Q, DORY_BACKWARD) != do16)) return DORY_OK;
        }
    sd->buf = c->send_buf;
    sd->row_ptr = p.d_send_map;
    sd->row_slots = p.d_send_map + c->N + 1;
    sd->w = wire.w;
    sd->R = (uint32_t)(wire.row_bytes() / sizeof(float));
    *bf16 = wire.bf16;
    fused_stamp_drop(c);   // (whatever a GEMM left in the send buffer is about to be overwritten)
    *send = true;
    return wait_halo(c);   // the previous exchange has finished reading the buffer
}
// defer_last (dory_gatmh_row_gather_overlap): the LAST exchange of the pass -- the merged one, or st's of the two -- is issued deferred where
// halo_overlap is set (counted); do's, the first of two, never: exchange_rows and the local transport hold ONE pending exchange
int gatmh_bwd_exchange(dory_ctx *c, Tensor *dO, Tensor *bgdo, Tensor *st, Tensor *bgst, bool producer_packed, bool defer_last) {
    const int on = sw_value(c, SW_GATMH_BWD_MERGED_EXCHANGE);
    if (transport_of(c) == Transport::Local)   // every rank ships one row format: checked before anything of this pass is enqueued or counted
        for (uint32_t q = 0; q < c->numNodes; ++q) {
            const dory_ctx *Q = q == c->nodeId ? nullptr : c->local->ctx[q];
            if (Q && sw_value(Q, SW_GATMH_BWD_MERGED_EXCHANGE) != on)
                return fail(c, DORY_ERR_COMM, "local transport: dory_gatmh_bwd_merged_exchange differs: rank %u has %d, rank %u has %d (all ranks must agree)",
                            c->nodeId, on, q, 1 - on);
        }
    if (gatmh_merged_taken(c)) {
        RowPair pair;
        pair.src2 = st; pair.ghost2 = bgst; pair.producer_packed = producer_packed;
        const int rc = exchange_rows(c, DORY_BACKWARD, dO, bgdo, defer_last, &pair);
        if (!rc && defer_last && c->halo_pending) c->gatmh_ovl_deferred++;
        return rc;
    }
    if (on == 1 && !c->capturing) c->count[CNT_MERGED_SPLIT_FALLBACKS]++;   // (the scatter transport: its own layout; halo_direct_recv: two tensors)
    int rc = exchange_rows(c, DORY_BACKWARD, dO, bgdo, false);   // (dory_gatmh_halo_bf16: do by the rule, st always fp32)
    if (!rc) rc = exchange_rows(c, DORY_BACKWARD, st, bgst, defer_last, nullptr, false);
    if (!rc && defer_last && c->halo_pending) c->gatmh_ovl_deferred++;
    return rc;
}

bool fused_pack_target(dory_ctx *c, const Tensor *out, uint32_t M, GemmSend *sd, int *dir) {
    if (!sw_on(c, SW_HALO_FUSED_PACK) || c->numNodes <= 1 || c->capturing || out->raw_handed || M != c->N || out->rows != c->N) return false;
    const Transport tr = transport_of(c);
    if (tr == Transport::Scatter || tr == Transport::None) return false;
    for (int d = 0; d < 2; ++d) {
        const HaloPlan &p = c->plan[d];
        if (!p.set || !p.d_send_map || p.send_map_rows != c->N || exchange_skipped(c, d) || (tr == Transport::Local && p.direct)) continue;
        for (uint32_t layer = 0; layer <= c->L; ++layer) {
            Tensor *src, *ghost;
            if (!halo_route(c, layer, d, &src, &ghost) || src != out || !ghost) continue;
            const RowWire wire = wire_shape(c, out, d);
            // dory_halo_bf16_rows: the pack kernel rounds the rows (no GEMM stores fp32 rows nobody sends) -- unless
            // dory_halo_fused_pack_bf16 has the epilogue round them; a wire row wider than the tensor's (one column, ld == 1) packs
            if (wire.bf16 && (!sw_on(c, SW_HALO_FUSED_PACK_BF16) || wire.w > out->ld)) return false;
            if ((size_t)p.send_total * wire.row_bytes() > c->send_cap) return false;   // (the exchange would regrow the buffer)
            sd->buf = c->send_buf;
            sd->row_ptr = p.d_send_map;
            sd->row_slots = p.d_send_map + c->N + 1;
            sd->w = wire.w;
            sd->bf16 = wire.bf16 ? 1u : 0u;
            *dir = d;
            return true;
        }
    }
    return false;
}
void fused_pack_stamp(dory_ctx *c, const Tensor *out, int dir, const GemmSend &sd, bool rowwise) {
    c->fused_stamp.src = out;
    c->fused_stamp.dir = dir;
    c->fused_stamp.w = sd.w;
    c->fused_stamp.buf = sd.buf;
    c->fused_stamp.bf16 = sd.bf16 != 0;
    c->fused_stamp.cols = sd.bf16 ? sd.cols : 0;
    c->fused_stamp.rowwise = rowwise;
}

// ---- bf16 ghost twins (dory_halo_bf16_ghosts) -----------------------------------------------------------------------------------
int ghost_fp32_current(dory_ctx *c, Tensor *t) {
    if (!t || !t->twin || t->twin_state != DORY_GHOST_TWIN) return DORY_OK;
    { int wrc = wait_halo(c); if (wrc) return wrc; }   // (the exchange that fills the twin may still be in flight)
    Timed tw(c, "bf16_widen", c->compute);
    HIPCK(c, launch_widen_rows_bf16(t->d, t->twin, t->rows * t->ld, c->compute));
    t->twin_state = DORY_GHOST_BOTH;
    if (!c->capturing) c->count[CNT_GHOST_WIDENED]++;
    if (!c->capturing && c->gnn == DORY_GATMH) c->count[CNT_GATMH_TWIN_WIDENED]++;
    return DORY_OK;
}

// every ghost tensor halo_route can ever name for a model whose exchanges may land bf16 (fg@0 comes from a file), where a row has at
// least one 8-byte quad; the multi-head GAT only with dory_gatmh_bf16_ghosts: fg_z and the bg_do of its own backward exchange (bg_st,
// fg_el, fg_er never: they travel and are read as fp32)
static bool ghost_gets_twin(const dory_ctx *c, uint32_t layer, const std::string &name, const Tensor &t) {
    if (!t.owned || t.ld < 4) return false;
    if (c->gnn == DORY_GATMH) return sw_on(c, SW_GATMH_BF16_GHOSTS) && !(t.ld & 7) && (name == "fg_z" || name == "bg_do");
    if (c->gnn == DORY_GCN) return (name == "fg" && layer >= 1) || name == "fgxw" || name == "bg" || name == "bgg";
    return c->gnn == DORY_GAT && (name == "fg_z" || name == "bg_d");
}
int ghost_twins_alloc(dory_ctx *c) {
    if (!sw_on(c, SW_HALO_BF16_GHOSTS)) return DORY_OK;
    for (uint32_t l = 0; l < c->tensors.size(); ++l)
        for (auto &kv : c->tensors[l]) {
            Tensor &t = kv.second;
            if (t.twin || !ghost_gets_twin(c, l, kv.first, t)) continue;
            const size_t b = t.twin_bytes() ? t.twin_bytes() : 256;   // (as alloc_tensor: a valid pointer for empty ghosts)
            HIPCK(c, hipMalloc((void **)&t.twin, b));
            HIPCK(c, hipMemsetAsync(t.twin, 0, b, c->compute));
            t.twin_state = DORY_GHOST_FP32;
        }
    return DORY_OK;
}
// (the merged row and the exchange of do alone ship bf16 by the same rule, gatmh_do_bf16; rows land in a twin as keeps_bf16 says)
bool gatmh_do_lands_in_twin(const dory_ctx *c, const Tensor *dO, const Tensor *bgdo) {
    return c->numNodes > 1 && sw_on(c, SW_HALO_BF16_GHOSTS) && bgdo->twin && !bgdo->raw_handed && gatmh_do_bf16(c, dO);
}

void scatter_free(dory_ctx *c) {
    ScatterState &S = c->scatter;
    scatter_drop_layouts(c, -1);
    for (void *p : {(void *)S.d_l2g, (void *)S.d_gvids[0], (void *)S.d_gvids[1], (void *)S.d_slot_row[0], (void *)S.d_slot_row[1], (void *)S.d_stamp[0],
                    (void *)S.d_stamp[1], (void *)S.d_counts[0], (void *)S.d_counts[1], (void *)S.d_stage[0], (void *)S.d_stage[1], (void *)S.d_send})
        if (p) (void)hipFree(p);
    for (void *p : {(void *)S.h_stage[0], (void *)S.h_stage[1], (void *)S.h_send})
        if (p) (void)hipHostFree(p);
    for (hipEvent_t e : {S.ev_stage[0], S.ev_stage[1]})
        if (e) (void)hipEventDestroy(e);
}

void epoch_graph_drop_locked(dory_ctx *c) {
    if (c->capturing) {   // abandon a recording in progress
        hipGraph_t g = nullptr;
        (void)hipStreamEndCapture(c->compute, &g);
        if (g) (void)hipGraphDestroy(g);
        c->capturing = false;
    }
    if (c->epoch_exec) (void)hipGraphExecDestroy(c->epoch_exec);
    if (c->epoch_graph) (void)hipGraphDestroy(c->epoch_graph);
    c->epoch_exec = nullptr;
    c->epoch_graph = nullptr;
    c->lr_table_left = 0;
}

// ---- the feature switches: one setter path and one reader of the counters (switches.hpp; the table: host/switches.cpp) ---------
// The hooks: what a switch does beyond its record, between the checks and the store.  A hook that fails leaves the switch as it was -- but the
// ghost twins' on path, which stores first (ghost_twins_alloc reads the switch): a failed allocation leaves it on, as it always did.
// dory_halo_fused_pack on: the send maps of the plans that exist already -- their lists come back from the device
static int fused_pack_hook(dory_ctx *c, SwitchId, int on) {
    for (int dir = 0; dir < 2 && on; ++dir) {
        HaloPlan &p = c->plan[dir];
        if (!p.set || p.d_send_map) continue;
        std::vector<uint32_t> lv(p.send_total);
        if (p.send_total) HIPCK(c, hipMemcpy(lv.data(), p.d_send_lvids, (size_t)p.send_total * sizeof(uint32_t), hipMemcpyDeviceToHost));
        int rc = build_send_map(c, p, lv.data());
        if (rc) return rc;
    }
    return DORY_OK;
}
// dory_gatmh_bwd_merged_exchange on, a backward plan that exists already: the buffers hold its widest merged rows from now on (no regrowth in an epoch)
static int merged_exchange_hook(dory_ctx *c, SwitchId, int on) {
    const HaloPlan &p = c->plan[DORY_BACKWARD];
    if (!on || c->numNodes <= 1 || !p.set || p.direct) return DORY_OK;
    const size_t rb = (size_t)gatmh_merged_row_max(c) * sizeof(float);
    const size_t sb = (size_t)p.send_total * rb, rcb = (size_t)p.recv_total * rb;
    if (c->local && (sb > c->send_cap || rcb > c->recv_cap))
        return fail(c, DORY_ERR_ARG, "gatmh_bwd_merged_exchange: the exchange buffers are too small for merged rows and the in-process peers hold "
                    "their addresses: call it before dory_comm_init_local");
    return ensure_exchange_buffers(c, sb, rcb);
}
// dory_halo_bf16_ghosts / dory_gatmh_bf16_ghosts.  On: the twins are allocated here (ghost_twins_alloc reads the switch: stored first).  Off: a twin that holds
// the only current copy is widened first; both streams idle, nothing in flight reads a twin; a recorded epoch may point at one; then every twin goes -- and the
// switch on top of the other goes off with either.
static int ghost_twins_hook(dory_ctx *c, SwitchId id, int on) {
    if (on) { c->sw[id].store(1, std::memory_order_release); return ghost_twins_alloc(c); }
    for (auto &m : c->tensors)
        for (auto &kv : m) { int rc = ghost_fp32_current(c, &kv.second); if (rc) return rc; }
    c->sw[id].store(0, std::memory_order_release);
    c->sw[SW_GATMH_BF16_GHOSTS].store(0, std::memory_order_release);
    HIPCK(c, hipStreamSynchronize(c->comm));
    HIPCK(c, hipStreamSynchronize(c->compute));
    epoch_graph_drop_locked(c);
    for (auto &m : c->tensors)
        for (auto &kv : m) {
            Tensor &t = kv.second;
            if (t.twin) (void)hipFree(t.twin);
            t.twin = nullptr;
            t.twin_state = DORY_GHOST_FP32;
        }
    return DORY_OK;
}
// the hook of every switch, by SwitchId (null: the record says it all): a new switch that owns memory adds its hook here
static int (*const SWITCH_HOOKS[])(dory_ctx *, SwitchId, int) = {
    fused_pack_hook, nullptr, nullptr, merged_exchange_hook, nullptr,   // halo_fused_pack, _bf16, _rowwise, gatmh_bwd_merged_exchange, gatmh_halo_bf16
    nullptr, ghost_twins_hook, ghost_twins_hook, nullptr, nullptr,      // halo_bf16_rows, halo_bf16_ghosts, gatmh_bf16_ghosts, gatmh_row_gather, _bf16
};
static_assert(sizeof(SWITCH_HOOKS) / sizeof(SWITCH_HOOKS[0]) == SW_COUNT && SW_HALO_FUSED_PACK == 0 && SW_GATMH_BWD_MERGED_EXCHANGE == 3 &&
              SW_HALO_BF16_GHOSTS == 6 && SW_GATMH_BF16_GHOSTS == 7, "switches: one hook slot per SwitchId, each hook at its switch's id");

// every dory_<switch>(ctx, value): the record's refusals in their order, what the record says a set does first, the hook, the store
static int switch_set(dory_ctx *c, SwitchId id, int value) {
    CHECK_CTX(c);
    const SwitchSpec &s = *switch_spec(id);
    char msg[320];
    if (switch_check(id, value, c->gnn, c->configured, c->prealloc, c->capturing, s.parent != SW_NONE && sw_on(c, (SwitchId)s.parent), msg, sizeof(msg)))
        return fail(c, DORY_ERR_ARG, "%s", msg);
    if (s.waits_halo) { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (s.drops_stamp) fused_stamp_drop(c);   // (rows a producer left for an exchange that may now ship another element, or not fuse)
    if (SWITCH_HOOKS[id]) { int rc = SWITCH_HOOKS[id](c, id, value); if (rc) return rc; }
    c->sw[id].store(value, std::memory_order_release);   // (the ghost twins' hook has stored it already: the same value again)
    return DORY_OK;
}
// every dory_<switch>_stats: the record's counters into the non-null pointers, in the order of the signature (n of them)
static int switch_stats(dory_ctx *c, SwitchId id, uint64_t *const out[], int n) {
    CHECK_CTX(c);
    const SwitchSpec &s = *switch_spec(id);
    for (int i = 0; i < n && i < s.ncounters; ++i)
        if (out[i]) *out[i] = c->count[s.counters[i]];
    if (s.twin_bytes && n > s.ncounters && out[s.ncounters]) {   // computed, not counted: the bytes of all bf16 twins
        *out[s.ncounters] = 0;
        for (auto &m : c->tensors)
            for (auto &kv : m)
                if (kv.second.twin) *out[s.ncounters] += kv.second.twin_bytes();
    }
    return DORY_OK;
}

}  // namespace dory

extern "C" {

int dory_comm_init_local(dory_ctx *const *ctxs, uint32_t n) {
    if (!ctxs || n < 2 || n > LOCAL_MAX_RANKS) return DORY_ERR_ARG;
    for (uint32_t i = 0; i < n; ++i) {
        dory_ctx *c = ctxs[i];
        if (!c) return DORY_ERR_ARG;
        std::lock_guard<std::mutex> lock(c->mu);
        if (!c->configured || c->numNodes != n || c->nodeId != i)
            return fail(c, DORY_ERR_ARG, "comm_init_local: context %u must be configured as rank %u of %u", i, i, n);
        if (c->device != ctxs[0]->device) return fail(c, DORY_ERR_ARG, "comm_init_local: all contexts on one device");
        if (!c->plan[0].set || !c->plan[1].set) return fail(c, DORY_ERR_ARG, "comm_init_local: halo plans first (dory_partition_upload / dory_halo_plan)");
        if (!c->prealloc) return fail(c, DORY_ERR_ARG, "comm_init_local: dory_preallocate first");
    }
    auto grp = std::make_shared<LocalGroup>();
    grp->ctx.assign(ctxs, ctxs + n);
    for (uint32_t i = 0; i < n; ++i) {
        dory_ctx *c = ctxs[i];
        std::lock_guard<std::mutex> lock(c->mu);
        HIPCK(c, hipSetDevice(c->device));
        HIPCK(c, hipStreamSynchronize(c->compute));
        HIPCK(c, hipStreamSynchronize(c->comm));
        for (hipEvent_t *e : {&c->ev_sent[0], &c->ev_sent[1], &c->ev_cons[0], &c->ev_cons[1], &c->ev_gready[0], &c->ev_gready[1],
                              &c->ev_gdone[0], &c->ev_gdone[1]})
            if (!*e) HIPCK(c, hipEventCreateWithFlags(e, hipEventDisableTiming));
        size_t need = 0;
        for (auto &m : c->wgrads)
            for (auto &kv : m) need = std::max(need, (size_t)kv.second.rows * kv.second.ld * sizeof(float));
        if (need > c->ar_tmp_cap) {
            if (c->ar_tmp) (void)hipFree(c->ar_tmp);
            c->ar_tmp = nullptr; c->ar_tmp_cap = 0;
            HIPCK(c, hipMalloc((void **)&c->ar_tmp, need));
            c->ar_tmp_cap = need;
        }
        c->posted_sent = 0; c->posted_cons = 0; c->posted_g = 0; c->posted_gdone = 0;
        c->local_seq = c->local_ar_seq = 0;
        c->local_pending = dory_ctx::LocalPending();
        c->local_sent_to.clear();
        fused_stamp_drop(c);
        c->local = grp;
    }
    return DORY_OK;
}

// ---------------------------------------------------------------------------------------
int dory_halo_plan(dory_ctx *c, int dir, const uint32_t *send_counts, const uint32_t *send_lvids,
                   const uint32_t *recv_counts, const uint32_t *recv_slots) {
    CHECK_CTX(c);
    if (!c->configured || !c->has_graph || (dir != 0 && dir != 1) || !send_counts || !recv_counts)
        return fail(c, DORY_ERR_ARG, "halo_plan: configure + graph_upload first / bad args");
    HaloPlan &p = c->plan[dir];
    const uint32_t P = c->numNodes;
    p.send_counts.assign(send_counts, send_counts + P);
    p.recv_counts.assign(recv_counts, recv_counts + P);
    p.send_off.assign(P + 1, 0);
    p.recv_off.assign(P + 1, 0);
    for (uint32_t i = 0; i < P; ++i) {
        p.send_off[i + 1] = p.send_off[i] + p.send_counts[i];
        p.recv_off[i + 1] = p.recv_off[i] + p.recv_counts[i];
    }
    p.send_total = p.send_off[P];
    p.recv_total = p.recv_off[P];
    const uint32_t G = c->adj[dir == DORY_FORWARD ? ADJ_IN : ADJ_OUT].ghosts;
    if (p.send_counts[c->nodeId] || p.recv_counts[c->nodeId]) return fail(c, DORY_ERR_ARG, "halo_plan: self entry must be empty");
    if (p.recv_total != G) return fail(c, DORY_ERR_ARG, "halo_plan: recv rows %u != ghost count %u", p.recv_total, G);
    for (uint32_t i = 0; i < p.send_total; ++i)
        if (send_lvids[i] >= c->N) return fail(c, DORY_ERR_ARG, "halo_plan: send lvid out of range");
    std::vector<char> seen(G, 0);
    for (uint32_t i = 0; i < p.recv_total; ++i) {
        if (recv_slots[i] >= G || seen[recv_slots[i]]) return fail(c, DORY_ERR_ARG, "halo_plan: recv slots must be a permutation of the ghost slots");
        seen[recv_slots[i]] = 1;
    }
    fused_stamp_drop(c);   // (the fused halo pack: slots of the old plan)
    if (p.d_send_lvids) (void)hipFree(p.d_send_lvids);
    if (p.d_unpack_slots && p.d_unpack_slots != p.d_recv_slots) (void)hipFree(p.d_unpack_slots);
    if (p.d_recv_slots) (void)hipFree(p.d_recv_slots);
    if (p.d_send_map) (void)hipFree(p.d_send_map);
    p.d_send_lvids = p.d_recv_slots = p.d_unpack_slots = p.d_send_map = nullptr;
    int rc;
    if ((rc = upload_array(c, &p.d_send_lvids, send_lvids, p.send_total))) return rc;
    if (sw_on(c, SW_HALO_FUSED_PACK) && (rc = build_send_map(c, p, send_lvids))) return rc;
    if ((rc = upload_array(c, &p.d_recv_slots, recv_slots, p.recv_total))) return rc;
    // option halo_direct_recv: received row r is ghost row r; recv_slots names the caller-visible index of that row (kept for
    // the uploads and downloads of ghost tensors), the unpack kernels get the identity
    p.direct = halo_direct(c);
    p.order.clear();
    p.d_unpack_slots = p.d_recv_slots;
    if (p.direct) {
        p.order.assign(recv_slots, recv_slots + p.recv_total);
        std::vector<uint32_t> ident(p.recv_total);
        std::iota(ident.begin(), ident.end(), 0u);
        p.d_unpack_slots = nullptr;
        if ((rc = upload_array(c, &p.d_unpack_slots, ident.data(), p.recv_total))) return rc;
    }
    p.set = true;
    scatter_drop_layouts(c, dir);   // (scatter messages: the message tables follow the send lists, the slot -> row map the wire order)
    if ((rc = scatter_slot_rows(c, dir))) return rc;
    // pack / receive buffers for the widest row any layer exchanges, now, so that no allocation (and no device-wide
    // synchronisation) happens inside an epoch
    uint32_t w = 0;
    for (uint32_t l = 0; l <= c->L; ++l) {
        w = std::max(w, pad_ld(c->dims[l]));
        if (c->gnn == DORY_GATMH && l < c->L && l < c->heads.size()) w = std::max(w, pad_ld(c->dims[l + 1] * c->heads[l]));
    }
    // (option halo_direct_recv: padded rows land in the ghost tensors; only exact rows narrower than their padding -- option
    // halo_exact_rows, as it stands now -- are staged)
    w = std::max(w, 2u);   // (dory_halo_bf16_rows: a one-column row travels as 4 bf16)
    if (c->gnn == DORY_GATMH && dir == DORY_BACKWARD && !p.direct && sw_on(c, SW_GATMH_BWD_MERGED_EXCHANGE))
        w = std::max(w, gatmh_merged_row_max(c));   // (dory_gatmh_bwd_merged_exchange: [do | st] rows)
    const bool staged = !p.direct || halo_exact(c);
    return ensure_exchange_buffers(c, (size_t)p.send_total * w * sizeof(float), staged ? (size_t)p.recv_total * w * sizeof(float) : 0);
}

int dory_comm_set_host_transport(dory_ctx *c, dory_alltoallv_fn alltoallv, dory_allreduce_fn allreduce_sum, void *user) {
    CHECK_CTX(c);
    if ((alltoallv == nullptr) != (allreduce_sum == nullptr)) return fail(c, DORY_ERR_ARG, "set_host_transport: both callbacks or none");
    fused_stamp_drop(c);
    c->tx_a2a = alltoallv;
    c->tx_ar = allreduce_sum;
    c->tx_user = user;
    c->scatter.fn = nullptr;   // (setting one transport clears the other)
    return DORY_OK;
}

int dory_comm_set_scatter_transport(dory_ctx *c, dory_scatter_exchange_fn exchange, dory_allreduce_fn allreduce_sum, void *user, uint64_t max_msg_bytes) {
    CHECK_CTX(c);
    if ((exchange == nullptr) != (allreduce_sum == nullptr)) return fail(c, DORY_ERR_ARG, "set_scatter_transport: both callbacks or none");
    if (max_msg_bytes > 0xFFFFFFFFull) return fail(c, DORY_ERR_ARG, "set_scatter_transport: max_msg_bytes %llu is not below 2^32", (unsigned long long)max_msg_bytes);
    fused_stamp_drop(c);
    c->scatter.fn = exchange;
    c->scatter.max_msg = max_msg_bytes;
    c->tx_a2a = nullptr;
    c->tx_ar = allreduce_sum;
    c->tx_user = user;
    if (!exchange) return DORY_OK;
    // the send buffers for the widest row any layer exchanges, now (as dory_halo_plan sizes the dense ones), where the plans exist
    uint32_t w = 1;
    for (uint32_t l = 0; l <= c->L && l < c->dims.size(); ++l) {
        w = std::max(w, c->dims[l]);
        if (c->gnn == DORY_GATMH && l < c->L && l < c->heads.size()) w = std::max(w, std::max(c->dims[l + 1], 4u) * c->heads[l]);
    }
    size_t need = 0;
    for (int dir = 0; dir < 2 && w <= scatter_msgs_max_cols(); ++dir) {
        if (!c->plan[dir].set) continue;
        const uint32_t batch = dory_wire_scatter_batch(w, max_msg_bytes);
        uint64_t end = 0;
        for (uint32_t q = 0; q < c->numNodes; ++q)
            for (uint32_t ib = 0; ib < c->plan[dir].send_counts[q]; ib += batch)
                end = ((end + 15ull) & ~15ull) + dory_wire_scatter_msg_bytes(std::min(batch, c->plan[dir].send_counts[q] - ib), w);
        need = std::max(need, (size_t)end);
    }
    return scatter_send_buffers(c, need);
}

int dory_comm_unique_id(void *id128) {
    if (!id128) return DORY_ERR_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return DORY_ERR_COMM;
    memcpy(id128, &id, sizeof(id));
    return DORY_OK;
}

int dory_comm_init(dory_ctx *c, const void *id128, int rank, int nranks) {
    CHECK_CTX(c);
    if (!id128 || rank < 0 || rank >= nranks) return fail(c, DORY_ERR_ARG, "comm_init: bad arguments");
    fused_stamp_drop(c);
    if (c->nccl) { ncclCommDestroy((ncclComm_t)c->nccl); c->nccl = nullptr; }
    ncclUniqueId id;
    memcpy(&id, id128, sizeof(id));
    ncclComm_t comm;
    NCCLCK(c, ncclCommInitRank(&comm, nranks, id, rank));
    c->nccl = comm;
    c->rank = rank;
    c->nranks = nranks;
    return DORY_OK;
}

int dory_halo_exchange(dory_ctx *c, uint32_t layer, int dir) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (c->numNodes == 1) return DORY_OK;  // no ghosts
    if (exchange_skipped(c, dir)) return DORY_OK;
    Tensor *src, *ghost;
    int rc = halo_tensors(c, layer, dir, &src, &ghost);
    if (rc) return rc;
    // a forward exchange of layer 0 rewrites fg@0 (a peer may have uploaded a new x): a cached ah@0 no longer holds
    if (layer == 0 && dir == DORY_FORWARD) c->ah0_valid = false;
    // consumers on the compute stream wait for the ghosts at once, or (halo_overlap) when the first of them needs
    // the ghost rows -- see wait_halo()
    return exchange_rows(c, dir, src, ghost, true);
}

// The split entry points: each does its own checks, then split_rows (the wire record, the "halo" interval, the kernels).
int dory_halo_pack(dory_ctx *c, uint32_t layer, int dir, float *send_buf) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *src, *ghost;
    int rc = halo_tensors(c, layer, dir, &src, &ghost);
    if (rc) return rc;
    if (!c->plan[dir].set) return fail(c, DORY_ERR_ARG, "halo_pack: no plan");
    return split_rows(c, "halo_pack", true, dir, src, ghost, send_buf, true);
}

int dory_halo_unpack(dory_ctx *c, uint32_t layer, int dir, const float *recv_buf) {
    CHECK_CTX(c);
    if (layer == 0) c->ah0_valid = false;   // (a caller's transport writing fg@0)
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *src, *ghost;
    int rc = halo_tensors(c, layer, dir, &src, &ghost);
    if (rc) return rc;
    if (!c->plan[dir].set) return fail(c, DORY_ERR_ARG, "halo_unpack: no plan");
    return split_rows(c, "halo_unpack", false, dir, src, ghost, const_cast<float *>(recv_buf), true);
}

// pack / unpack of any named tensor with the plan of `dir`
int dory_halo_pack_tensor(dory_ctx *c, uint32_t layer, const char *name, int dir, float *send_buf) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *src = name ? find(c, layer, name) : nullptr;
    if (!src || (dir != 0 && dir != 1) || !c->plan[dir].set) return fail(c, DORY_ERR_ARG, "halo_pack_tensor: no tensor '%s'@%u or no plan", name ? name : "(null)", layer);
    if (src->rows != c->N) return fail(c, DORY_ERR_ARG, "halo_pack_tensor: '%s' is not a per-local-vertex tensor", name);
    return split_rows(c, "halo_pack_tensor", true, dir, src, nullptr, send_buf, false);
}

int dory_halo_unpack_tensor(dory_ctx *c, uint32_t layer, const char *name, int dir, const float *recv_buf) {
    CHECK_CTX(c);
    if (layer == 0) c->ah0_valid = false;   // (a caller's transport writing fg@0)
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *ghost = name ? find(c, layer, name) : nullptr;
    if (!ghost || (dir != 0 && dir != 1) || !c->plan[dir].set) return fail(c, DORY_ERR_ARG, "halo_unpack_tensor: no tensor '%s'@%u or no plan", name ? name : "(null)", layer);
    if (ghost->rows != c->adj[dir == DORY_FORWARD ? ADJ_IN : ADJ_OUT].ghosts) return fail(c, DORY_ERR_ARG, "halo_unpack_tensor: '%s' is not a ghost tensor of that direction", name);
    if (!strcmp(name, "fg_z") && layer < c->gat_nsum_valid.size()) c->gat_nsum_valid[layer] = 0;   // (as halo_tensors: the kept neighbour sum of the old ghost rows no longer holds)
    return split_rows(c, "halo_unpack_tensor", false, dir, nullptr, ghost, const_cast<float *>(recv_buf), false);
}

// ---- the fused halo pack: switch and counters (include/dorylus_hip.h) ----------------------------------------------------------
int dory_halo_fused_pack(dory_ctx *c, int on) { return switch_set(c, SW_HALO_FUSED_PACK, on); }
int dory_halo_fused_pack_stats(dory_ctx *c, uint64_t *fused_exchanges, uint64_t *fused_rows, uint64_t *fallback_exchanges) {
    uint64_t *const out[] = {fused_exchanges, fused_rows, fallback_exchanges};
    return switch_stats(c, SW_HALO_FUSED_PACK, out, 3);
}

// dory_halo_fused_pack_bf16: the fused pack also serves the exchanges that ship bf16 rows (K2's send16 kernels)
int dory_halo_fused_pack_bf16(dory_ctx *c, int on) { return switch_set(c, SW_HALO_FUSED_PACK_BF16, on); }
int dory_halo_fused_pack_bf16_stats(dory_ctx *c, uint64_t *fused_bf16_exchanges, uint64_t *fused_bf16_rows) {
    uint64_t *const out[] = {fused_bf16_exchanges, fused_bf16_rows};
    return switch_stats(c, SW_HALO_FUSED_PACK_BF16, out, 2);
}

// dory_halo_fused_pack_rowwise: the fused pack also serves the exchanges whose source a row-wise kernel writes (the send forms of
// csrc/elementwise.hip; dory_apply_vertex and dory_predict_gat launch them)
int dory_halo_fused_pack_rowwise(dory_ctx *c, int on) { return switch_set(c, SW_HALO_FUSED_PACK_ROWWISE, on); }
int dory_halo_fused_pack_rowwise_stats(dory_ctx *c, uint64_t *rowwise_exchanges, uint64_t *rowwise_rows) {
    uint64_t *const out[] = {rowwise_exchanges, rowwise_rows};
    return switch_stats(c, SW_HALO_FUSED_PACK_ROWWISE, out, 2);
}

// ---- the multi-head GAT's merged backward exchange: switch, counters, and the split entry points (include/dorylus_hip.h) ----------
int dory_gatmh_bwd_merged_exchange(dory_ctx *c, int on) { return switch_set(c, SW_GATMH_BWD_MERGED_EXCHANGE, on); }
int dory_gatmh_bwd_merged_exchange_stats(dory_ctx *c, uint64_t *merged_exchanges, uint64_t *merged_rows, uint64_t *producer_packed, uint64_t *split_fallbacks) {
    uint64_t *const out[] = {merged_exchanges, merged_rows, producer_packed, split_fallbacks};
    return switch_stats(c, SW_GATMH_BWD_MERGED_EXCHANGE, out, 4);
}

// the tensors of the three split entry points after their checks: DORY_GATMH, preallocated, a backward plan, `layer` the tensors' layer
static int gatmh_bwd_split(dory_ctx *c, const char *who, uint32_t layer, Tensor **dO, Tensor **st, Tensor **bgdo, Tensor **bgst, RowWire *wire) {
    if (!c->configured || c->gnn != DORY_GATMH || !c->prealloc || !c->plan[DORY_BACKWARD].set)
        return fail(c, DORY_ERR_ARG, "%s: a DORY_GATMH context after dory_preallocate with a backward plan", who);
    if (layer >= c->L) return fail(c, DORY_ERR_ARG, "%s: layer %u out of range", who, layer);
    *dO = find(c, layer, "do"); *st = find(c, layer, "st"); *bgdo = find(c, layer, "bg_do"); *bgst = find(c, layer, "bg_st");
    if (!*dO || !*st || !*bgdo || !*bgst) return fail(c, DORY_ERR_ARG, "%s: tensors missing", who);
    *wire = pair_wire(c, *dO, *st, gatmh_do_bf16(c, *dO));
    return DORY_OK;
}

int dory_gatmh_bwd_wire_row(dory_ctx *c, uint32_t layer, uint32_t *row_floats, uint32_t *do_floats, uint32_t *st_floats) {
    CHECK_CTX(c);
    Tensor *dO, *st, *bgdo, *bgst;
    RowWire wire;
    int rc = gatmh_bwd_split(c, "gatmh_bwd_wire_row", layer, &dO, &st, &bgdo, &bgst, &wire);
    if (rc) return rc;
    if (row_floats) *row_floats = (uint32_t)(wire.row_bytes() / sizeof(float));
    if (do_floats) *do_floats = wire.bf16 ? wire.w / 2 : wire.w;   // (4-byte units: w bf16 are w / 2 of them)
    if (st_floats) *st_floats = wire.w2;
    return DORY_OK;
}

int dory_gatmh_bwd_wire_do(dory_ctx *c, uint32_t layer, uint32_t *elem_bytes, uint32_t *elems) {
    CHECK_CTX(c);
    Tensor *dO, *st, *bgdo, *bgst;
    RowWire wire;
    int rc = gatmh_bwd_split(c, "gatmh_bwd_wire_do", layer, &dO, &st, &bgdo, &bgst, &wire);
    if (rc) return rc;
    if (elem_bytes) *elem_bytes = wire.elem_bytes();
    if (elems) *elems = wire.w;
    return DORY_OK;
}

// ---- dory_gatmh_halo_bf16: the multi-head GAT under the rule of dory_halo_bf16_rows (halo_ships_bf16) -------------------------------
int dory_gatmh_halo_bf16(dory_ctx *c, int on) { return switch_set(c, SW_GATMH_HALO_BF16, on); }
int dory_gatmh_halo_bf16_stats(dory_ctx *c, uint64_t *fwd_bf16_exchanges, uint64_t *bwd_bf16_exchanges, uint64_t *bwd_bf16_rows, uint64_t *producer_packed_bf16) {
    uint64_t *const out[] = {fwd_bf16_exchanges, bwd_bf16_exchanges, bwd_bf16_rows, producer_packed_bf16};
    return switch_stats(c, SW_GATMH_HALO_BF16, out, 4);
}

int dory_gatmh_bwd_pack(dory_ctx *c, uint32_t layer, float *send_buf) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *dO, *st, *bgdo, *bgst;
    RowWire wire;
    int rc = gatmh_bwd_split(c, "gatmh_bwd_pack", layer, &dO, &st, &bgdo, &bgst, &wire);
    if (rc) return rc;
    const HaloPlan &p = c->plan[DORY_BACKWARD];
    if (p.send_total && (!send_buf || ((uintptr_t)send_buf & 15))) return fail(c, DORY_ERR_ARG, "gatmh_bwd_pack: a 16-byte aligned device buffer");
    Timed t(c, "halo", c->compute);
    return pack_rows(c, send_buf, dO, wire, p, c->compute, st);   // (dory_gatmh_halo_bf16: the do part by the rule of this moment)
}

int dory_gatmh_bwd_unpack(dory_ctx *c, uint32_t layer, const float *recv_buf) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *dO, *st, *bgdo, *bgst;
    RowWire wire;
    int rc = gatmh_bwd_split(c, "gatmh_bwd_unpack", layer, &dO, &st, &bgdo, &bgst, &wire);
    if (rc) return rc;
    const HaloPlan &p = c->plan[DORY_BACKWARD];
    if (bgdo->rows != p.recv_total || bgst->rows != p.recv_total)
        return fail(c, DORY_ERR_ARG, "gatmh_bwd_unpack: ghost tensors of %llu rows for a plan that receives %u", (unsigned long long)bgdo->rows, p.recv_total);
    if (p.recv_total && (!recv_buf || ((uintptr_t)recv_buf & 15))) return fail(c, DORY_ERR_ARG, "gatmh_bwd_unpack: a 16-byte aligned device buffer");
    Timed t(c, "halo", c->compute);
    const bool keep = keeps_bf16(c, wire, bgdo);   // (dory_gatmh_bf16_ghosts: the do part stays bf16 in bg_do's twin)
    rc = unpack_rows(c, bgdo->d, bgdo->ld, wire, recv_buf, p, c->compute, keep ? bgdo->twin : nullptr, bgst->d, bgst->ld);
    ghost_wrote_fp32(bgst);
    return rc ? rc : ghost_rows_landed(c, bgdo, keep, false, c->compute, true, DORY_BACKWARD, true);
}

// ---- bf16 halo rows: switch, counters, and the row an exchange puts on the wire (include/dorylus_hip.h) ------------------------
int dory_halo_bf16_rows(dory_ctx *c, int on) { return switch_set(c, SW_HALO_BF16_ROWS, on); }
int dory_halo_bf16_rows_stats(dory_ctx *c, uint64_t *bf16_packs, uint64_t *bf16_bytes, uint64_t *fp32_packs_while_on) {
    uint64_t *const out[] = {bf16_packs, bf16_bytes, fp32_packs_while_on};
    return switch_stats(c, SW_HALO_BF16_ROWS, out, 3);
}

int dory_halo_wire_row(dory_ctx *c, uint32_t layer, int dir, uint32_t *elem_bytes, uint32_t *row_elems) {
    CHECK_CTX(c);
    if (!c->configured || !c->prealloc || (dir != 0 && dir != 1)) return fail(c, DORY_ERR_ARG, "halo_wire_row: configure + preallocate first; dir is 0 or 1");
    Tensor *src, *ghost;
    if (!halo_route(c, layer, dir, &src, &ghost)) return fail(c, DORY_ERR_ARG, "halo_wire_row: layer %u out of range", layer);
    if (!src || !ghost) return fail(c, DORY_ERR_ARG, "halo_wire_row: tensors missing");
    RowWire wire;
    int rc = row_wire(c, "halo_wire_row", src, ghost, true, nullptr, dir, &wire);
    if (rc) return rc;
    if (elem_bytes) *elem_bytes = wire.elem_bytes();
    if (row_elems) *row_elems = wire.w;
    return DORY_OK;
}

// ---- bf16 ghost twins: switch, counters, and a look at one tensor's twin (include/dorylus_hip.h) ---------------------------------
int dory_halo_bf16_ghosts(dory_ctx *c, int on) { return switch_set(c, SW_HALO_BF16_GHOSTS, on); }
int dory_halo_bf16_ghosts_stats(dory_ctx *c, uint64_t *landed_direct, uint64_t *landed_by_kernel, uint64_t *conversions_skipped, uint64_t *widened, uint64_t *twin_bytes) {
    uint64_t *const out[] = {landed_direct, landed_by_kernel, conversions_skipped, widened, twin_bytes};
    return switch_stats(c, SW_HALO_BF16_GHOSTS, out, 5);
}

int dory_halo_bf16_ghost_peek(dory_ctx *c, uint32_t layer, const char *name, const void **twin, int *state) {
    CHECK_CTX(c);
    Tensor *t = name ? find(c, layer, name) : nullptr;
    if (!t) return fail(c, DORY_ERR_ARG, "halo_bf16_ghost_peek: no tensor '%s' at layer %u", name ? name : "(null)", layer);
    { int wrc = wait_halo(c); if (wrc) return wrc; }   // (a deferred exchange: its rows are enqueued before the caller looks; dory_sync waits for them)
    if (twin) *twin = t->twin;
    if (state) *state = t->twin_state;
    return DORY_OK;
}

// ---- dory_gatmh_bf16_ghosts: twins for the multi-head GAT's fg_z and bg_do, on top of dory_halo_bf16_ghosts ------------------------
int dory_gatmh_bf16_ghosts(dory_ctx *c, int on) { return switch_set(c, SW_GATMH_BF16_GHOSTS, on); }
int dory_gatmh_bf16_ghosts_stats(dory_ctx *c, uint64_t *fwd_kept, uint64_t *bwd_kept, uint64_t *bwd_kept_merged, uint64_t *twin_reads_rows,
                                 uint64_t *twin_reads_sweep, uint64_t *scores_from_twin, uint64_t *widened) {
    uint64_t *const out[] = {fwd_kept, bwd_kept, bwd_kept_merged, twin_reads_rows, twin_reads_sweep, scores_from_twin, widened};
    return switch_stats(c, SW_GATMH_BF16_GHOSTS, out, 7);
}

// ---- dory_gatmh_row_gather: the switch of the row-gather family (gat_mh_rows.hip) and its pass counters (include/dorylus_hip.h) ----
int dory_gatmh_row_gather(dory_ctx *c, int mode) { return switch_set(c, SW_GATMH_ROW_GATHER, mode); }
int dory_gatmh_row_gather_stats(dory_ctx *c, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *dst_rowwise, uint64_t *src) {
    uint64_t *const out[] = {fwd, dst_edge_pass, dst_rowwise, src};
    return switch_stats(c, SW_GATMH_ROW_GATHER, out, 4);
}

// ---- dory_gatmh_row_gather_bf16: option gatmh_bf16_gather reaches the row-gather family (its bf16 forms), and the passes that ran one ----
int dory_gatmh_row_gather_bf16(dory_ctx *c, int on) { return switch_set(c, SW_GATMH_ROW_GATHER_BF16, on); }
int dory_gatmh_row_gather_bf16_stats(dory_ctx *c, uint64_t *fwd, uint64_t *dst_edge_pass, uint64_t *src) {
    uint64_t *const out[] = {fwd, dst_edge_pass, src};
    return switch_stats(c, SW_GATMH_ROW_GATHER_BF16, out, 3);
}

// ---- scatter messages: the entry points (helpers above) ------------------------------------------------------------------
int dory_halo_wire_ids(dory_ctx *c, const uint32_t *local_to_global, const uint32_t *src_ghost_gvids, const uint32_t *dst_ghost_gvids) {
    CHECK_CTX(c);
    if (!c->configured || !c->has_graph) return fail(c, DORY_ERR_ARG, "halo_wire_ids: configure + graph_upload first");
    if (c->N && !local_to_global) return fail(c, DORY_ERR_ARG, "halo_wire_ids: no local_to_global");
    const uint32_t *gv[2] = {src_ghost_gvids, dst_ghost_gvids};
    for (int dir = 0; dir < 2; ++dir) {
        const uint32_t G = ghost_count(c, dir);
        if (G && !gv[dir]) return fail(c, DORY_ERR_ARG, "halo_wire_ids: no ghost ids of dir %d (%u ghosts)", dir, G);
        for (uint32_t k = 1; k < G; ++k)
            if (gv[dir][k - 1] >= gv[dir][k])
                return fail(c, DORY_ERR_ARG, "halo_wire_ids: the ghost ids of dir %d are not ascending (slot %u: %u, then %u)", dir, k - 1, gv[dir][k - 1], gv[dir][k]);
    }
    ScatterState &S = c->scatter;
    HIPCK(c, hipDeviceSynchronize());
    for (uint32_t **p : {&S.d_l2g, &S.d_gvids[0], &S.d_gvids[1], &S.d_stamp[0], &S.d_stamp[1], &S.d_counts[0], &S.d_counts[1]}) {
        if (*p) (void)hipFree(*p);
        *p = nullptr;
    }
    S.ids = false;
    int rc;
    if ((rc = upload_array(c, &S.d_l2g, local_to_global, c->N))) return rc;
    for (int dir = 0; dir < 2; ++dir) {
        const uint32_t G = ghost_count(c, dir);
        S.gvids[dir].assign(gv[dir], gv[dir] + G);
        if ((rc = upload_array(c, &S.d_gvids[dir], gv[dir], G))) return rc;
        HIPCK(c, hipMalloc((void **)&S.d_stamp[dir], G ? (size_t)G * sizeof(uint32_t) : 256));
        HIPCK(c, hipMemset(S.d_stamp[dir], 0, G ? (size_t)G * sizeof(uint32_t) : 256));
        HIPCK(c, hipMalloc((void **)&S.d_counts[dir], 256));
        HIPCK(c, hipMemset(S.d_counts[dir], 0, 256));
        S.round[dir] = 1;
    }
    // the staging area of dory_scatter_msgs_deliver, once: a reference message (1 MiB) or the widest record any layer exchanges
    uint32_t w = 1;
    for (uint32_t l = 0; l <= c->L && l < c->dims.size(); ++l) {
        w = std::max(w, c->dims[l]);
        if (c->gnn == DORY_GATMH && l < c->L && l < c->heads.size()) w = std::max(w, std::max(c->dims[l + 1], 4u) * c->heads[l]);
    }
    const size_t stage = std::max<size_t>(DORY_WIRE_MAX_MSG_SIZE, ((size_t)4 * (1 + w) + 4095) & ~(size_t)4095);
    if (stage > S.stage_bytes) {
        for (int i = 0; i < 2; ++i) {
            if (S.h_stage[i]) (void)hipHostFree(S.h_stage[i]);
            if (S.d_stage[i]) (void)hipFree(S.d_stage[i]);
            S.h_stage[i] = S.d_stage[i] = nullptr;
        }
        S.stage_bytes = 0;
        for (int i = 0; i < 2; ++i) {
            HIPCK(c, hipHostMalloc((void **)&S.h_stage[i], stage, hipHostMallocDefault));
            HIPCK(c, hipMalloc((void **)&S.d_stage[i], stage));
            if (!S.ev_stage[i]) HIPCK(c, hipEventCreateWithFlags(&S.ev_stage[i], hipEventDisableTiming));
            S.stage_used[i] = false;
        }
        S.stage_bytes = stage;
    }
    S.ids = true;
    for (int dir = 0; dir < 2; ++dir)
        if ((rc = scatter_slot_rows(c, dir))) return rc;
    return DORY_OK;
}

// (layer, dir, name) -> the source tensor of a pack and the layer its messages name
static int scatter_source(dory_ctx *c, const char *who, uint32_t layer, int dir, const char *name, Tensor **src, uint32_t *hdr_layer) {
    if (dir != 0 && dir != 1) return fail(c, DORY_ERR_ARG, "%s: dir %d", who, dir);
    if (name) {
        *src = find(c, layer, name);
        if (!*src) return fail(c, DORY_ERR_ARG, "%s: no tensor '%s'@%u", who, name, layer);
        if ((*src)->rows != c->N) return fail(c, DORY_ERR_ARG, "%s: '%s' is not a per-local-vertex tensor", who, name);
        *hdr_layer = layer;
        return DORY_OK;
    }
    Tensor *ghost;
    int rc = halo_tensors(c, layer, dir, src, &ghost);
    if (rc) return rc;
    *hdr_layer = tensor_layer(c, ghost);
    return DORY_OK;
}

int dory_scatter_msgs_layout(dory_ctx *c, uint32_t layer, int dir, const char *name, uint64_t max_msg_bytes, struct dory_scatter_msg *msgs,
                             uint32_t max_msgs, uint32_t *n_msgs, uint64_t *total_bytes) {
    CHECK_CTX(c);
    Tensor *src;
    uint32_t hdr_layer;
    int rc = scatter_source(c, "scatter_msgs_layout", layer, dir, name, &src, &hdr_layer);
    if (rc) return rc;
    ScatterLayout *L;
    if ((rc = scatter_layout(c, "scatter_msgs_layout", dir, src->cols, max_msg_bytes, false, &L))) return rc;
    if (n_msgs) *n_msgs = (uint32_t)L->msgs.size();
    if (total_bytes) *total_bytes = L->total_bytes;
    if (msgs) {
        if (max_msgs < L->msgs.size()) return fail(c, DORY_ERR_ARG, "scatter_msgs_layout: %zu messages, room for %u", L->msgs.size(), max_msgs);
        std::copy(L->msgs.begin(), L->msgs.end(), msgs);
    }
    return DORY_OK;
}

int dory_scatter_msgs_pack(dory_ctx *c, uint32_t layer, int dir, const char *name, uint64_t max_msg_bytes, void *dev_buf) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    Tensor *src;
    uint32_t hdr_layer;
    int rc = scatter_source(c, "scatter_msgs_pack", layer, dir, name, &src, &hdr_layer);
    if (rc) return rc;
    Timed t(c, "halo", c->compute);
    return scatter_pack(c, "scatter_msgs_pack", dir, src, hdr_layer, max_msg_bytes, dev_buf, c->compute, nullptr);
}

int dory_scatter_msgs_deliver(dory_ctx *c, const char *name, const void *const *msgs, const uint64_t *bytes, uint32_t n) {
    if (!c) return DORY_ERR_ARG;
    // from the scatter transport's callback (the thread that runs the exchange holds the lock) or from anywhere else
    const bool in_cb = c->scatter.in_cb.load(std::memory_order_acquire) && c->scatter.cb_thread == std::this_thread::get_id();
    std::unique_lock<std::mutex> lock(c->mu, std::defer_lock);
    if (!in_cb) {
        lock.lock();
        HIPCK(c, hipSetDevice(c->device));
        int wrc = wait_halo(c);
        if (wrc) return wrc;
    }
    return scatter_deliver(c, name, msgs, bytes, n, in_cb);
}

int dory_scatter_msgs_unpack(dory_ctx *c, uint32_t layer, int dir, const char *name, const void *dev_records, uint32_t count) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    const char *who = "scatter_msgs_unpack";
    ScatterState &S = c->scatter;
    if (dir != 0 && dir != 1) return fail(c, DORY_ERR_ARG, "%s: dir %d", who, dir);
    if (!S.ids || !c->plan[dir].set) return fail(c, DORY_ERR_ARG, "%s: dory_halo_wire_ids and a plan first", who);
    Tensor *src = nullptr, *ghost = nullptr;
    if (name) ghost = find(c, layer, name);
    else { int rc = halo_tensors(c, layer, dir, &src, &ghost); if (rc) return rc; }
    if (!ghost) return fail(c, DORY_ERR_ARG, "%s: no tensor '%s'@%u", who, name, layer);
    if (ghost->rows != ghost_count(c, dir) || ghost->rows != S.gvids[dir].size())
        return fail(c, DORY_ERR_ARG, "%s: the tensor is not a ghost tensor of dir %d", who, dir);
    if (ghost->cols > scatter_msgs_max_cols()) return fail(c, DORY_ERR_ARG, "%s: rows of %u floats (scatter messages carry 1 .. %u)", who, ghost->cols, scatter_msgs_max_cols());
    if (count && (!dev_records || ((uintptr_t)dev_records & 15))) return fail(c, DORY_ERR_ARG, "%s: the records must be 16-byte aligned", who);
    const uint32_t tl = tensor_layer(c, ghost);
    if (ghost == find(c, 0, "fg")) c->ah0_valid = false;
    if (ghost == find(c, tl, "fg_z") && tl < c->gat_nsum_valid.size()) c->gat_nsum_valid[tl] = 0;
    ghost_wrote_fp32(ghost);   // (dory_halo_bf16_ghosts: records are fp32; a round writes every ghost row)
    HIPCK(c, hipEventRecord(c->ev_a, c->compute));
    HIPCK(c, hipStreamWaitEvent(c->comm, c->ev_a, 0));
    Timed t(c, "halo", c->comm);
    HIPCK(c, launch_scatter_msgs_unpack(ghost->d, ghost->ld, ghost->cols, dev_records, count, S.d_gvids[dir], (uint32_t)S.gvids[dir].size(), S.d_slot_row[dir],
                                        S.d_stamp[dir], S.round[dir], S.d_counts[dir], c->comm));
    return DORY_OK;
}

int dory_scatter_msgs_finish(dory_ctx *c, uint32_t layer, int dir, const char *name, uint32_t *rows, uint32_t *unknown, uint32_t *duplicate) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (dir != 0 && dir != 1) return fail(c, DORY_ERR_ARG, "scatter_msgs_finish: dir %d", dir);
    if (!c->scatter.ids) return fail(c, DORY_ERR_ARG, "scatter_msgs_finish: dory_halo_wire_ids first");
    if (name && !find(c, layer, name)) return fail(c, DORY_ERR_ARG, "scatter_msgs_finish: no tensor '%s'@%u", name, layer);
    return scatter_finish(c, dir, rows, unknown, duplicate);
}

// ---------------------------------------------------------------------------------------
// The validation statistics of the last forward pass summed over all partitions: what WeightServer::updateLocalAccLoss /
// updateGlobalAccLoss do with the AccLoss records the graph servers send (src/weight-server/weightserver.cpp:190-262:
// vtcsCnt, acc and loss added up over the nodes, then "Epoch %u, acc: %.4f, loss: %.4f" on node 0).  Every rank calls it
// (a collective); every rank gets the sums.
int dory_train_stat_global(dory_ctx *c, float *acc_sum, float *loss_sum, uint32_t *val_rows) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (!c->d_stat3) return fail(c, DORY_ERR_ARG, "train_stat_global: context not created properly");
    float h[3] = {0.f, 0.f, 0.f};
    HIPCK(c, hipMemcpyAsync(h, c->d_stat, 2 * sizeof(float), hipMemcpyDeviceToHost, c->compute));
    HIPCK(c, hipStreamSynchronize(c->compute));
    h[2] = (float)c->val_rows;      // (exact below 2^24 rows per sum: Friendster's 6.6 M validation rows fit)
    if (c->numNodes > 1 && (transport_of(c) == Transport::Host || transport_of(c) == Transport::Scatter)) {   // the three floats are on the host already
        if (c->tx_ar(c->tx_user, h, 3)) return fail(c, DORY_ERR_COMM, "train_stat_global: host transport allreduce failed");
    } else if (c->numNodes > 1) {
        HIPCK(c, hipMemcpyAsync(c->d_stat3, h, sizeof(h), hipMemcpyHostToDevice, c->compute));
        int rc = allreduce_sum(c, "train_stat_global", c->d_stat3, 3, [&](dory_ctx *Q) -> const float * {
            if (!Q->d_stat3) fail(c, DORY_ERR_COMM, "local transport: rank %u has no statistics buffer", Q->nodeId);
            return Q->d_stat3;
        });
        if (rc) return rc;
        HIPCK(c, hipMemcpyAsync(h, c->d_stat3, sizeof(h), hipMemcpyDeviceToHost, c->compute));
        HIPCK(c, hipStreamSynchronize(c->compute));
    }
    if (acc_sum) *acc_sum = h[0];
    if (loss_sum) *loss_sum = h[1];
    if (val_rows) *val_rows = (uint32_t)(h[2] + 0.5f);
    return DORY_OK;
}

// ---------------------------------------------------------------------------------------
int dory_adam_config(dory_ctx *c, float learning_rate) {
    CHECK_CTX(c);
    c->adam.lr = learning_rate;
    c->adam.epochs = 1;
    c->lr_table_left = 0;   // an epoch graph's step-size table is refilled on its next launch
    return DORY_OK;
}

int dory_weight_update(dory_ctx *c, uint32_t layer) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (!c->prealloc || layer >= c->L) return fail(c, DORY_ERR_ARG, "weight_update: bad state or layer");
    const float lr_t = adam_lr_t(c, c->adam.epochs);
    for (auto &kv : c->weights[layer]) {
        const std::string &name = kv.first;
        // the reference only updates "w"; a_i updates are faked on the weight server
        // (src/weight-server/weightserver.cpp:112-116) -- keep a_i fixed as it does.
        if (name != "w" && c->gnn != DORY_GATMH) continue;   // the extension trains a_l / a_r too
        Tensor &w = kv.second;
        Tensor &g = c->wgrads[layer][name];
        const uint64_t n = (uint64_t)w.rows * w.ld;
        if (c->numNodes > 1) {
            auto peer_grad = [&](dory_ctx *Q) -> const float * {   // rank Q's gradient of this weight
                if (layer >= Q->wgrads.size()) {
                    fail(c, DORY_ERR_COMM, "local transport: rank %u has no layer %u", Q->nodeId, layer);
                    return nullptr;
                }
                auto it = Q->wgrads[layer].find(name);
                if (it != Q->wgrads[layer].end() && (uint64_t)it->second.rows * it->second.ld == n) return it->second.d;
                fail(c, DORY_ERR_COMM, "local transport: rank %u's gradient '%s'@%u has another shape", Q->nodeId, name.c_str(), layer);
                return nullptr;
            };
            // (refused before the interval opens: no communicator leaves no "allreduce" timing entry)
            if (transport_of(c) == Transport::None) return fail(c, DORY_ERR_COMM, "weight_update: dory_comm_init not called");
            Timed t(c, "allreduce", c->compute);
            int rc = allreduce_sum(c, "weight_update", g.d, n, peer_grad);
            if (rc) return rc;
        }
        Timed t(c, "adam", c->compute);
        if (c->capturing)   // replayed epochs: step size from the table dory_epoch_graph_launch fills
            HIPCK(c, launch_adam_table(w.d, g.d, c->adam_m[layer][name].d, c->adam_v[layer][name].d, n, c->d_lr_table,
                                       c->d_replay_idx, c->compute));
        else
            HIPCK(c, launch_adam(w.d, g.d, c->adam_m[layer][name].d, c->adam_v[layer][name].d, n, lr_t, c->compute));
    }
    if (layer == 0 && !c->capturing) {   // "if(layer == 0) nextIteration();" (AdamOptimizer.cpp:49-50)
        c->adam.epochs += 1;
        c->lr_table_left = 0;            // eager step: a recorded epoch's table no longer lines up
    }
    return DORY_OK;
}

// ---------------------------------------------------------------------------------------
// Epoch graph: one epoch of C-ABI calls recorded into a hipGraph and replayed, so that a
// launch-bound epoch (Cora-sized graphs: ~35 kernels of a few microseconds) costs one
// graph launch.  No reference counterpart; single partition only (the exchange is not
// recorded).  Everything an epoch allocates lazily must exist already: run one eager epoch
// first.  Per-epoch host scalars do not survive recording, so Adam's step size comes from a
// device table indexed by a replay counter that the graph's last node bumps.
int dory_epoch_graph_drop(dory_ctx *c) {
    CHECK_CTX(c);
    epoch_graph_drop_locked(c);
    return DORY_OK;
}

int dory_epoch_graph_begin(dory_ctx *c) {
    CHECK_CTX(c);
    if (!c->prealloc) return fail(c, DORY_ERR_ARG, "epoch_graph_begin: preallocate first");
    if (c->numNodes > 1) return fail(c, DORY_ERR_ARG, "epoch graph: single partition only (the halo exchange is not recorded)");
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch_graph_begin: already recording");
    epoch_graph_drop_locked(c);
    if (!c->d_replay_idx) HIPCK(c, hipMalloc((void **)&c->d_replay_idx, 256));
    if (!c->d_lr_table) {
        c->lr_table_cap = 1024;
        HIPCK(c, hipMalloc((void **)&c->d_lr_table, c->lr_table_cap * sizeof(float)));
    }
    HIPCK(c, hipStreamSynchronize(c->compute));
    HIPCK(c, hipStreamBeginCapture(c->compute, hipStreamCaptureModeThreadLocal));
    c->capturing = true;
    return DORY_OK;
}

int dory_epoch_graph_end(dory_ctx *c) {
    CHECK_CTX(c);
    if (!c->capturing) return fail(c, DORY_ERR_ARG, "epoch_graph_end: not recording");
    hipError_t e = launch_bump_counter(c->d_replay_idx, c->compute);
    hipGraph_t g = nullptr;
    hipError_t e2 = hipStreamEndCapture(c->compute, &g);
    c->capturing = false;
    if (e != hipSuccess || e2 != hipSuccess || !g) {
        if (g) (void)hipGraphDestroy(g);
        return fail(c, DORY_ERR_HIP, "epoch_graph_end: recording failed (%s)", hipGetErrorString(e != hipSuccess ? e : e2));
    }
    c->epoch_graph = g;
    e = hipGraphInstantiate(&c->epoch_exec, g, nullptr, nullptr, 0);
    if (e != hipSuccess) {
        c->epoch_exec = nullptr;
        epoch_graph_drop_locked(c);
        return fail(c, DORY_ERR_HIP, "epoch_graph_end: hipGraphInstantiate failed (%s)", hipGetErrorString(e));
    }
    return DORY_OK;
}

int dory_epoch_graph_launch(dory_ctx *c, uint32_t epochs) {
    CHECK_CTX(c);
    if (!c->epoch_exec) return fail(c, DORY_ERR_ARG, "epoch_graph_launch: no recorded epoch");
    for (uint32_t i = 0; i < epochs; ++i) {
        if (c->lr_table_left == 0) {
            // step sizes of the next replays, a pure function of the iteration count: filled well
            // ahead so that the host copy + counter reset happen once per lr_table_cap epochs
            HIPCK(c, hipStreamSynchronize(c->compute));   // previous replays have read the old table
            c->lr_table_host.resize(c->lr_table_cap);
            for (uint32_t k = 0; k < c->lr_table_cap; ++k) c->lr_table_host[k] = adam_lr_t(c, c->adam.epochs + k);
            // on the replay stream itself: c->compute is a non-blocking stream, the legacy null stream is not ordered
            // against it (a null-stream memset could still be in flight when the replayed adam_table_kernel reads *idx)
            HIPCK(c, hipMemcpyAsync(c->d_lr_table, c->lr_table_host.data(), c->lr_table_cap * sizeof(float), hipMemcpyHostToDevice, c->compute));
            HIPCK(c, hipMemsetAsync(c->d_replay_idx, 0, sizeof(uint32_t), c->compute));
            HIPCK(c, hipStreamSynchronize(c->compute));   // lr_table_host may be resized again only after the copy
            c->lr_table_left = c->lr_table_cap;
        }
        HIPCK(c, hipGraphLaunch(c->epoch_exec, c->compute));
        c->lr_table_left -= 1;
        c->adam.epochs += 1;
    }
    return DORY_OK;
}

}  // extern "C"
