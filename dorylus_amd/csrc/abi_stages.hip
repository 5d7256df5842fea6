// abi_stages.hip -- C-ABI, part 2: the stage dispatch that replaces the reference's Engine::aggregate* bodies and
// ResourceComm::NNCompute (aggregate, apply_vertex, apply_edge, predict, validation statistics).
#include "abi_internal.hpp"

namespace dory {
// ---------------------------------------------------------------------------------------
// the blocked copy a multi-head GAT layer of leading dimension ld gathers through
static BlockedAdj &gatmh_blocked_for(Adjacency &A, uint32_t ld) { return ld < 128 && A.blk16.built ? A.blk16 : A.blk; }

// K1b bookkeeping: (re)build the source-blocked copy of one adjacency for `group` lanes/row
int ensure_blocked(dory_ctx *c, Adjacency &A, int group, bool narrow_set) {
    DerivedAdj &B = narrow_set ? A.blk16 : A.blk;
    const uint32_t want_nb = (uint32_t)c->opt[OPT_SPMM_BLK_NB];
    // the block structure serves every slab width; only an explicit block count forces a rebuild
    const bool rebuild = B.built && want_nb && B.nb != (want_nb + 7) / 8 * 8;
    if (c->capturing && (!B.built || rebuild) && !A.blk.na)
        return fail(c, DORY_ERR_ARG, "epoch graph: blocked adjacency would have to be (re)built while recording");
    if (rebuild) {
        HIPCK(c, hipStreamSynchronize(c->compute));
        free_blocked(&B);
        B.built = false;
    }
    if (!B.built) {
        const uint32_t NG = c->N + A.ghosts;
        // K1b pays nb partial rows per output row: only worth it (and only affordable: the
        // per-(block,row) offset table is nb*(N+1) words) while the source space is a few
        // hundred L2 windows at most.  Larger partitions keep K1.
        const uint64_t window = 0;   // K1b's own windows (K1s has its own layout: ensure_sweep)
        const uint32_t nb = plan_blocks(NG, want_nb, (uint32_t)group * 16u, window);
        // ... and pointless when the whole source slab fits one XCD's L2 anyway (Cora-sized graphs):
        // K1 then gathers from L2 without partial sums or a second kernel
        // (a partitioned multi-head GAT run has no row-wise form that reads ghost rows: it always takes the blocks)
        const bool tiny = !want_nb && (uint64_t)NG * group * 16u <= ((uint64_t)4 << 20) &&
                          !(c->gnn == DORY_GATMH && c->numNodes > 1);
        if (tiny || nb > 256 || (uint64_t)nb * (c->N + 1) * 8ull > ((uint64_t)8 << 30)) {
            if (!narrow_set) A.blk.na = true;   // (no second copy: the narrow layers share the first)
            return DORY_OK;
        }
        HIPCK(c, build_blocked(A.ptr, A.idx, A.val, c->N, NG, A.nnz, want_nb, (uint32_t)group * 16u, &B, c->compute, window));
        B.row_bytes = (uint32_t)group * 16u;
        B.built = true;
    }
    return DORY_OK;
}

// K1s bookkeeping: the even layout build_blocked_sweep makes of one adjacency (spmm.hip)
int ensure_sweep(dory_ctx *c, Adjacency &A, int group) {
    DerivedAdj &S = A.swp;
    const uint32_t want_nb = (uint32_t)c->opt[OPT_SPMM_BLK_NB];
    if (S.built && S.want_nb != want_nb && !c->capturing) {   // another block count requested (tests): rebuild
        HIPCK(c, hipStreamSynchronize(c->compute));
        free_blocked(&S);
        S.built = false;
    }
    if (S.built || S.na) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: the sweep layout would have to be built while recording");
    const uint32_t NG = c->N + A.ghosts;
    // the deal is made for the 32-lane launches; the multi-head GAT passes keep ten registers per row: 4 rows at most
    int R;
    if (c->gnn == DORY_GATMH) {
        // four rows while that fills every CU at least once (fewer sweeps = fewer refills of every window: 4.47 -> 4.17 ms per
        // 128-float forward launch from two rows to four); small partitions pick by fill
        const uint32_t G_ = std::min<uint32_t>(32u, c->cus_per_xcd);
        const int forced = (int)c->opt[OPT_GATMH_SWEEP_ROWS];
        R = (!forced && c->N >= 8u * G_ * 32u * 4u) ? 4 : sweep_pick_r(c->N, 32, G_, forced, 4);
    } else {
        R = sweep_pick_r(c->N, 32, std::min<uint32_t>(32u, c->cus_per_xcd), (int)c->opt[OPT_SPMM_SWEEP_ROWS]);
    }
    // source window per block.  0 = by the rows a lane group holds: a step costs ~3 us whatever it gathers, and a small
    // partition (one rank of 8: four rows per group) gathers little per step -- fewer, larger windows win there although
    // two of them no longer fit the L2 (measured, one rank of 8 of the Reddit-size graph: 2432 / 3072 / 3584 / 4096 / 5120 KB
    // = 3.34 / 3.22 / 3.16 / 3.21 / 3.38 ms per epoch; ranks of 4, 2 and the whole graph: 2432 KB stays best)
    // (multi-head GAT contexts: their sweeps carry 13-17 vector instructions per gather and two to four rows per group, and run
    // best on 4.5 MB windows -- 128-float forward 4.45 / 4.16 / 4.09 / 4.29 / 4.88 ms at 2432 / 3584 / 4608 / 6144 / 8192 KB)
    // (round 6: the 8-head GAT's SOURCE side gathers a 128-byte statistics record beside every 512-byte row -- its window is a
    // quarter larger than the forward's for the same rows, and at 4.5 MB of rows it ran fabric-bound: 29.6 GB fetched in 5.1 ms
    // per 128-float launch; the out-edge layout therefore gets its own window, option gatmh_src_window_kb)
    const bool out_edges = &A == &c->adj[ADJ_OUT];   // (by identity: an Adjacency is only ever handed on by reference into c->adj)
    const uint64_t gat_kb = (c->gnn == DORY_GATMH && out_edges && c->opt[OPT_GATMH_SRC_WINDOW_KB]) ? (uint64_t)c->opt[OPT_GATMH_SRC_WINDOW_KB] : 4608u;
    const uint64_t window_kb = c->opt[OPT_SPMM_SWEEP_WINDOW_KB] ? (uint64_t)c->opt[OPT_SPMM_SWEEP_WINDOW_KB]
                                                              : (c->gnn == DORY_GATMH && R >= 4 ? gat_kb : (R <= 4 ? 3584u : 2432u));
    const uint64_t window = window_kb << 10;
    const uint64_t nb_est = ((uint64_t)NG * group * 16u + window - 1) / window + 1;
    // the whole source slab in one L2 (Cora-sized graphs): K1 gathers from L2 anyway.  Thousands of windows (Amazon-,
    // Friendster-sized partitions on a random graph: a row has a fraction of an edge per window): the per-(block,
    // position) offset table alone would be nb*(N+1) words -- K1
    const bool tiny = !want_nb && (uint64_t)NG * group * 16u <= ((uint64_t)4 << 20);
    if (tiny || c->N < 8 || (want_nb ? want_nb : nb_est) > 512 || (want_nb ? want_nb : nb_est) * (uint64_t)(c->N + 1) * 8ull > ((uint64_t)8 << 30)) {
        S.na = true;
        return DORY_OK;
    }
    HIPCK(c, build_blocked_sweep(A.ptr, A.idx, A.val, c->N, NG, A.nnz, want_nb, (uint32_t)group * 16u, window, R, &S, c->compute,
                                 (uint32_t)c->opt[OPT_SPMM_SWEEP_LAYOUT], std::min<uint32_t>(32u, c->cus_per_xcd),
                                 group == 32 && c->opt[OPT_SPMM_SWEEP_LOADER] ? (uint32_t)c->opt[OPT_SPMM_SWEEP_LOADER_RELIEF] : 0u));
    S.want_nb = want_nb;
    S.built = true;
    return DORY_OK;
}

int blk_group_for(dory_ctx *c, uint32_t ld) {
    int group = (int)c->opt[OPT_SPMM_BLK_GROUP];
    if (group != 8 && group != 16 && group != 32) group = 32;
    if (ld < 128 && group == 32) group = 16;   // narrow tensors: one 256-B slab
    return group;
}

// Options gcn_bf16_gather / gatmh_bf16_gather, dory_gat_bf16_gather: the rows of one aggregation rounded to bf16 into the context's shadow buffer,
// [N local rows ; ghost rows], every call (nothing is kept: a caller may write x / h / fg through a raw pointer between two
// calls).  The buffer only grows, outside a recording.
static int bf16_reserve(dory_ctx *c, uint64_t rows, uint32_t ld, const char *option) {
    const size_t need = (size_t)rows * ld * sizeof(uint16_t);
    if (need <= c->bf16_rows_bytes) return DORY_OK;
    if (c->capturing) return fail(c, DORY_ERR_ARG, "epoch graph: the bf16 rows of %s would have to grow while recording", option);
    if (c->bf16_rows) {
        HIPCK(c, hipStreamSynchronize(c->compute));
        (void)hipFree(c->bf16_rows);
        c->bf16_rows = nullptr;
        c->bf16_rows_bytes = 0;
        epoch_graph_drop_locked(c);   // (a recorded epoch would read the freed buffer)
    }
    HIPCK(c, hipMalloc((void **)&c->bf16_rows, need));
    c->bf16_rows_bytes = need;
    return DORY_OK;
}
static int bf16_convert(dory_ctx *c, const Tensor &t, uint64_t first_row) {
    if (!t.rows) return DORY_OK;
    Timed tc(c, "bf16_convert", c->compute);
    HIPCK(c, launch_bf16_rows(t.d, c->bf16_rows + first_row * t.ld, t.rows * t.ld, c->compute));
    return DORY_OK;
}
// One aggregation's use of the shadow buffer.  begin() sizes it and converts the N local rows at once: xl / xg are what the
// kernels' row pointers become.  The ghost rows are converted by ghosts_landed(), to be called once the exchange that writes
// them has landed (after wait_halo; at once where they have landed already).  Never begun = fp32 rows: nothing to convert.
struct Bf16Rows {
    dory_ctx *c = nullptr;
    const Tensor *ghost = nullptr;
    const float *xl = nullptr, *xg = nullptr;   // bf16 rows of ld elements; xg == nullptr: no ghost rows
    bool from_twin = false;                     // xg is the ghost tensor's twin (dory_gatmh_bf16_ghosts_stats counts by it)
    // dory_halo_bf16_ghosts: where the ghost tensor's bf16 twin is current (the exchange landed its rows there) the ghost rows are
    // the twin itself -- only the N local rows are reserved and converted, ghosts_landed() has nothing to do (counted).  Not for a
    // tensor whose raw pointer is out: the caller may have written its fp32 rows since (they are kept current: state BOTH), so those
    // are converted as ever
    int begin(dory_ctx *ctx, const Tensor &rows, const Tensor *ghost_rows, uint64_t nghost, const char *option) {
        Tensor local = rows;
        local.rows = ctx->N;
        const bool twin = nghost && ghost_rows->twin_current() && !ghost_rows->raw_handed;
        int rc = bf16_reserve(ctx, (uint64_t)ctx->N + (twin ? 0 : nghost), rows.ld, option);
        if (!rc) rc = bf16_convert(ctx, local, 0);
        if (rc) return rc;
        c = ctx;
        ghost = nghost && !twin ? ghost_rows : nullptr;
        xl = reinterpret_cast<const float *>(c->bf16_rows);
        xg = !nghost ? nullptr : twin ? reinterpret_cast<const float *>(ghost_rows->twin)
                                      : reinterpret_cast<const float *>(c->bf16_rows + (size_t)c->N * rows.ld);
        from_twin = twin;
        if (twin && !c->capturing) c->count[CNT_GHOST_CONVERSIONS_SKIPPED]++;
        return DORY_OK;
    }
    bool on() const { return c != nullptr; }
    int ghosts_landed() { return ghost ? bf16_convert(c, *ghost, c->N) : DORY_OK; }
};

// The schedule every kernel family of spmm() follows around a halo exchange: what does not read the ghost rows is launched
// `first`, timed as "spmm_beside_halo" (under an exchange in flight; "spmm_local_first": the same split with nothing in
// flight), then the compute stream waits for the ghosts (and rounds them, for an aggregation on bf16 rows), then `rest` runs.
// Not split: the wait, then `rest` alone.  bf == nullptr: an aggregation on fp32 rows (K1b has no other).
template <class First, class Rest>
static int around_halo(dory_ctx *c, bool split, Bf16Rows *bf, First first, Rest rest) {
    int rc;
    if (split) {
        Timed tb(c, c->halo_pending ? "spmm_beside_halo" : "spmm_local_first", c->compute);
        if ((rc = first())) return rc;
    }
    if ((rc = wait_halo(c)) || (bf && (rc = bf->ghosts_landed()))) return rc;
    return rest();
}

// What a launch sequence on the sweep skeleton (K1s, the 8-head GAT's edge passes) needs beside its tensors, decided once per
// aggregation; part() is one launch of it.
struct SweepLaunch {
    int group = 32;             // lanes per row
    int R = 0;                  // rows per lane group: the actual count, whichever family
    uint32_t G = 32;            // workgroups per sweep and XCD
    // With ghost rows the blocks that hold local rows only always run as a launch of their own (they do not
    // depend on an exchange in flight), so the overlapped and the sequential schedule are the same arithmetic.
    bool two = false;
    bool bf16 = false, wide = false;   // the rows gathered: bf16 rows; eight features per lane (its own groups and slabs)
    SweepCtl ctl;
    uint32_t sflags = 0;        // option spmm_sweep_flags, + 8 (ungated) where the XCD placement check failed and "gated" was not measured faster
    size_t need = 0;            // bytes of gate counters the larger of its launches takes
    uint32_t *done = nullptr;   // the counters (c->partial); nullptr: c->partial holds fewer than `need` bytes
    hipStream_t s = nullptr;
    SweepPart part(uint32_t b_lo, uint32_t b_hi, bool accumulate, uint32_t reserve = 0) const {
        return SweepPart{G, b_lo, b_hi, accumulate, reserve, R, done, ctl, sflags, s, bf16, wide};
    }
};
static uint32_t sweep_flags(dory_ctx *c) {
    return (uint32_t)c->opt[OPT_SPMM_SWEEP_FLAGS] | (((!c->xcd_mapping_ok || c->opt[OPT_SPMM_XCD_ASSUME_MISMATCH]) && c->xcd_policy != 0) ? 8u : 0u);
}
static SweepLaunch sweep_launch(dory_ctx *c, const BlockedAdj &S, uint32_t ld, int group, bool ghosts, int R, bool bf16, bool wide) {
    SweepLaunch sw;
    sw.group = group;
    sw.R = R;
    sw.G = std::min<uint32_t>(32u, c->cus_per_xcd);
    sw.two = ghosts && S.nb_local > 0 && S.nb_local < S.nb;
    sw.bf16 = bf16;
    sw.wide = wide;
    sw.ctl = SweepCtl{(int)c->opt[OPT_SPMM_SWEEP_PAIR], c->opt[OPT_SPMM_SWEEP_LOADER] != 0, c->sweep_stat};   // (pair, loader: K1s's forms)
    sw.sflags = sweep_flags(c);
    sw.need = sweep_counter_bound(S.npos, ld, group, R, wide, sw.G, sw.two ? std::max(S.nb_local, S.nb - S.nb_local) : S.nb);
    sw.done = sw.need <= c->partial_bytes ? reinterpret_cast<uint32_t *>(c->partial) : nullptr;
    sw.s = c->compute;
    return sw;
}

// K1s's rows per lane group on `group` lanes (the wide form: 16) of the layout S: option spmm_sweep_rows, else what S was dealt for
int k1s_rows(dory_ctx *c, const BlockedAdj &S, int group) {
    return sweep_rows(S.rows_per_group, S.npos, group, std::min<uint32_t>(32u, c->cus_per_xcd), (int)c->opt[OPT_SPMM_SWEEP_ROWS]);
}

// K1s's placement check failed (ctx.hpp): gates would synchronise workgroups that do not share an L2.  Decide once per context,
// by measurement, on a launch that may be repeated (it writes, does not accumulate): gated against ungated.  The three probe
// launches are timed under their own key ("spmm_xcd_probe"), outside the caller's "spmm" region.
static int xcd_probe(dory_ctx *c, const SpmmArgs &a, const BlockedAdj &S, const float *row_scale, const SweepLaunch &sw) {
    struct Ev3 {   // destroyed on every way out (HIPCK returns)
        hipEvent_t e[3] = {nullptr, nullptr, nullptr};
        ~Ev3() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    Timed tp(c, "spmm_xcd_probe", c->compute);
    for (auto &x : ev.e) HIPCK(c, hipEventCreate(&x));
    SweepPart p = sw.part(0, sw.two ? S.nb_local : S.nb, false);
    const uint32_t gated = sw.sflags & ~8u;
    for (int i = 0; i < 3; ++i) {   // ungated (warm: layout, code), gated, ungated
        p.flags = i == 1 ? gated : gated | 8u;
        HIPCK(c, launch_spmm_sweep(a, S, sw.group, row_scale, c->scratch, p));
        HIPCK(c, hipEventRecord(ev.e[i], c->compute));
    }
    HIPCK(c, hipEventSynchronize(ev.e[2]));
    (void)hipEventElapsedTime(&c->xcd_gated_ms, ev.e[0], ev.e[1]);
    (void)hipEventElapsedTime(&c->xcd_ungated_ms, ev.e[1], ev.e[2]);
    c->xcd_policy = c->xcd_gated_ms <= c->xcd_ungated_ms ? 0 : 8;
    return DORY_OK;
}

constexpr int SPMM_NOT_MINE = 1;   // spmm_k1s / spmm_k1b: this aggregation goes to the next kernel family

// K1s: register accumulators, every workgroup sweeps all source blocks of its own even layout (spmm.hip).
static int spmm_k1s(dory_ctx *c, Adjacency &A, const SpmmArgs &a, const float *row_scale, Bf16Rows &bf) {
    const int group = blk_group_for(c, a.ld);
    int rc = ensure_sweep(c, A, group);
    if (rc) return rc;
    const DerivedAdj &S = A.swp;
    if (S.na || !sweep_supported(a, S, group)) return SPMM_NOT_MINE;
    const bool bf16 = bf.on();
    // option gcn_bf16_wide (GAT prototype: dory_gat_bf16_gather's `wide`): bf16 rows of 128 floats or more are gathered eight
    // features per lane (same bits; spmm.hip)
    const bool gat = c->gnn == DORY_GAT;
    const bool wide = bf16 && (gat ? c->gat_bf16_wide : c->opt[OPT_GCN_BF16_WIDE] == 1) && sweep_wide_applies(a.ld, group, k1s_rows(c, S, 16));
    SweepLaunch sw = sweep_launch(c, S, a.ld, group, a.xg != nullptr, k1s_rows(c, S, wide ? 16 : group), bf16, wide);
    if ((rc = ensure_partial(c, sw.need, "sweep counters"))) return rc;   // (K1s may still size its counters here, outside a recording)
    sw.done = reinterpret_cast<uint32_t *>(c->partial);
    if (S.nslots && (rc = ensure_scratch(c, (size_t)S.nslots * a.ld * sizeof(float)))) return rc;   // pieces of split rows
    c->last_spmm_unit = row_scale != nullptr;
    if ((!c->xcd_mapping_ok || c->opt[OPT_SPMM_XCD_ASSUME_MISMATCH]) && !(c->opt[OPT_SPMM_SWEEP_FLAGS] & 8) && c->xcd_policy < 0 &&
        !c->capturing && !a.accumulate && !c->halo_pending) {
        if ((rc = xcd_probe(c, a, S, row_scale, sw))) return rc;
        sw.sflags = sweep_flags(c);   // (left undecided -- recording, accumulating caller: ungated, never a timeout)
    }
    Timed t(c, "spmm", c->compute);
    c->spmm_launches_k1s++;
    if (bf16) (gat ? c->gat_bf16_gathers_k1s : c->bf16_gathers_k1s)++;
    if (wide) (gat ? c->gat_bf16_gathers_k1s_wide : c->bf16_gathers_k1s_wide)++;
    auto sweep = [&](const SweepPart &p) -> int {
        HIPCK(c, launch_spmm_sweep(a, S, group, row_scale, c->scratch, p));
        return DORY_OK;
    };
    // under an exchange in flight the RCCL kernels need CUs of their own; the ghost-source blocks go on from the first launch's sums
    const uint32_t reserve = c->halo_pending ? (uint32_t)c->opt[OPT_SPMM_SWEEP_RESERVE_CUS] : 0u;
    rc = around_halo(c, sw.two, &bf, [&] { return sweep(sw.part(0, S.nb_local, false, reserve)); },
                     [&] { return sweep(sw.two ? sw.part(S.nb_local, S.nb, true) : sw.part(0, S.nb, false)); });
    if (rc) return rc;
    HIPCK(c, launch_spmm_sweep_combine(a, S, row_scale, c->scratch, c->compute, bf16));
    return DORY_OK;
}

// K1b: partial rows per source block, then a reduce (spmm_blocked.hip).  No bf16 form.
static int spmm_k1b(dory_ctx *c, Adjacency &A, const SpmmArgs &a, const float *row_scale) {
    const int group = blk_group_for(c, a.ld);
    int rc = ensure_blocked(c, A, group);
    if (rc) return rc;
    const DerivedAdj &B = A.blk;
    const size_t need = blocked_partial_bytes(a, B);
    if (B.na || B.nb == 0 || need > ((size_t)48 << 30)) return SPMM_NOT_MINE;
    c->last_spmm_unit = row_scale != nullptr;
    if ((rc = ensure_partial(c, need, "partial buffer"))) return rc;
    Timed t(c, "spmm", c->compute);
    c->spmm_launches_k1b++;
    auto part = [&](uint32_t b_lo, uint32_t b_hi) -> int {
        HIPCK(c, launch_spmm_blocked_part(a, B, c->partial, group, row_scale != nullptr, b_lo, b_hi, c->compute));
        return DORY_OK;
    };
    // source blocks that contain local rows only do not depend on the exchange in
    // flight: they run first, the ghost blocks after the comm stream's event
    const uint32_t nb_local = std::min(B.nb, c->N / B.SB);
    const bool split = (c->halo_pending || c->opt[OPT_SPMM_BLK_FORCE_SPLIT]) && nb_local > 0 && nb_local < B.nb;
    if ((rc = around_halo(c, split, nullptr, [&] { return part(0, nb_local); }, [&] { return part(split ? nb_local : 0, B.nb); }))) return rc;
    if (B.nchunks) {   // hubs: the remainder of the (block,row) segments K1b stopped in
        if ((rc = ensure_scratch(c, (size_t)B.nchunks * a.ld * sizeof(float)))) return rc;
        HIPCK(c, launch_spmm_blocked_long_segments(a, B, c->partial, row_scale != nullptr, c->scratch, c->compute));
    }
    HIPCK(c, launch_spmm_blocked_reduce(a, B, c->partial, row_scale, c->compute));
    return DORY_OK;
}

// K1: the row gather with per-edge values (spmm.hip), whatever the graph.
static int spmm_k1(dory_ctx *c, Adjacency &A, SpmmArgs a, Bf16Rows &bf) {
    if (!a.val) return fail(c, DORY_ERR_ARG, "spmm: no edge values");
    const bool bf16 = bf.on();
    c->spmm_launches_k1++;
    if (bf16) (c->gnn == DORY_GAT ? c->gat_bf16_gathers_k1 : c->bf16_gathers_k1)++;
    // dory_k1_bf16_wide: every launch of this aggregation gathers its bf16 rows 16 bytes a lane where the rule has a form for the row
    // and slab width and the shadow rows and the ghost rows (the twin, or the shadow rows' tail) are 16-byte aligned; else narrow, counted
    bool wide = false;
    if (bf16 && c->k1_bf16_wide) {
        uint32_t lanes, chunks;
        const int64_t slab = c->opt[OPT_SPMM_SLAB];
        wide = k1_rows8_form(a.ld, slab > 0 ? (uint32_t)slab : 0u, &lanes, &chunks) &&
               !((reinterpret_cast<uintptr_t>(a.xl) | reinterpret_cast<uintptr_t>(a.xg)) & 15);
        (wide ? c->k1_rows8_wide : c->k1_rows8_narrow)++;
    }
    auto launch = [&](const SpmmArgs &x) -> int {
        HIPCK(c, launch_spmm(x, (int)c->opt[OPT_SPMM_SLAB], c->compute, bf16, wide));
        return DORY_OK;
    };
    const LongRowsDev &longRows = A.long_rows;
    if (longRows.nchunks) {   // hubs: K1 stops after LONG_ROW_CLAMP edges of a row, workgroup-per-chunk kernels do the rest
        int rc = ensure_scratch(c, (size_t)longRows.nchunks * a.ld * sizeof(float));
        if (rc) return rc;
        a.row_clamp = LONG_ROW_CLAMP;
    }
    const bool in_flight = c->halo_pending || c->opt[OPT_SPMM_BLK_FORCE_SPLIT];
    // K1 under an exchange in flight.  GCN partitions with ghosts hold a local-first copy of the edges (ctx.hpp: EdgeSplit): one
    // launch sums every row's local-source edges beside the exchange, a second one goes on from those sums with the ghost-
    // source edges (boundary rows only) -- the additions happen in the same order as in ONE launch over the copy, which is what
    // runs when nothing is in flight: overlapped and sequential schedule give the same bits.
    const EdgeSplit &es = A.edge_split;
    // (layer 0's forward aggregation reads ghost rows that came from a file: no exchange ever precedes it, in either schedule,
    // so it keeps the reference's edge order -- the local-first copy costs the 300-float Amazon launch a few per cent)
    if (es.idx && a.xg && a.val == A.val && !longRows.nchunks && !a.accumulate && c->opt[OPT_SPMM_EDGE_SPLIT] && !c->agg_static_ghosts) {
        a.idx = es.idx;
        a.val = es.val;
        Timed t(c, "spmm", c->compute);
        SpmmArgs p1 = a, p2 = a;
        p1.ptr_end = es.mid;
        p2.ptr = es.mid;
        p2.ptr_end = a.ptr + 1;
        p2.self_mode = 0;
        p2.accumulate = 2;
        const bool boundary = !A.split || A.n_interior < c->N;   // rows without a ghost source are done
        if (A.split && boundary) { p2.order = A.split + A.n_interior; p2.rows = c->N - A.n_interior; }
        return around_halo(c, in_flight, &bf, [&] { return launch(p1); },
                           [&] { return !in_flight ? launch(a) : boundary ? launch(p2) : (int)DORY_OK; });
    }
    // (other cases -- GAT's per-epoch edge values, hub rows: the rows whose sources are all local run first, the rows that read
    // ghost rows after the comm stream's event)
    const bool split_rows = in_flight && A.split && A.n_interior > 0 && A.n_interior < c->N && !longRows.nchunks;
    Timed t(c, "spmm", c->compute);
    SpmmArgs interior = a, boundary = a;
    if (split_rows) {
        interior.order = A.split;
        interior.rows = A.n_interior;
        boundary.order = A.split + A.n_interior;
        boundary.rows = c->N - A.n_interior;
    }
    return around_halo(c, split_rows, &bf, [&] { return launch(interior); }, [&]() -> int {
        if (split_rows) return launch(boundary);
        int rc = launch(a);
        if (!rc && longRows.nchunks) HIPCK(c, launch_spmm_long_rows(a, longRows, c->scratch, c->compute, bf16));
        return rc;
    });
}

// One aggregation.  Edge weights come from `val` (any per-edge array, K1), or -- when
// `val` is the adjacency's own static array -- from the source-blocked copy (K1b), or are
// 1 with a per-destination factor `row_scale` (K1b, unit mode; the reference GAT's edge
// scores depend on the destination only, CPU_comm.cpp:299-319).
// bf16 (option gcn_bf16_gather; GAT prototype: dory_gat_bf16_gather): every row read -- self row, local and ghost rows -- is
// rounded to bf16 first; edge values, norm, row_scale, the sums and `out` stay fp32, the sums in the order of the fp32 path.
// K1s and K1 have bf16 forms, K1b has none: where fp32 would take K1b, bf16 takes K1.  row_scale on bf16 rows: the GAT
// prototype's unit-weight forms of K1s only.  bf_out (optional): the aggregation's shadow rows, for a caller that reads the
// rounded self rows once more (they stay until the next aggregation on bf16 rows).
static int spmm(dory_ctx *c, Adjacency &A, const float *val, int self_mode, Tensor &xl, Tensor *xg, Tensor &out,
                uint32_t F, int accumulate, const float *row_scale = nullptr, bool bf16 = false, Bf16Rows *bf_out = nullptr) {
    if (xl.ld != out.ld || (xg && xg->rows && xg->ld != xl.ld) || xl.cols != F)
        return fail(c, DORY_ERR_ARG, "spmm: tensor shapes disagree (F=%u ld %u/%u)", F, xl.ld, out.ld);
    if (bf16 && ((row_scale && c->gnn != DORY_GAT) || xl.rows < c->N))
        return fail(c, DORY_ERR_ARG, "spmm: bf16 rows need edge weights (but on a GAT context) and N rows");
    c->last_spmm_unit = false;
    // dory_halo_bf16_ghosts: an aggregation on fp32 rows of a ghost tensor whose twin alone is current (the gather mode changed after
    // the exchange) gets the twin widened first; one on bf16 rows reads the twin itself (Bf16Rows::begin)
    if (!bf16 && xg && xg->rows) { int grc = ghost_fp32_current(c, xg); if (grc) return grc; }
    SpmmArgs a{};
    a.N = c->N; a.F = F; a.ld = xl.ld;
    a.ptr = A.ptr;
    a.idx = A.idx;
    a.val = val;
    a.self_scale = c->norm;
    a.self_mode = self_mode;
    a.xl = xl.d; a.xg = (xg && xg->rows) ? xg->d : nullptr; a.out = out.d;   // nullptr: no ghost rows (the blocked kernel then skips the select)
    Bf16Rows bf;
    if (bf16) {   // the kernels' xl / xg point at bf16 rows from here on
        int rc = bf.begin(c, xl, xg, a.xg ? xg->rows : 0, c->gnn == DORY_GAT ? "dory_gat_bf16_gather" : "gcn_bf16_gather");
        if (rc) return rc;
        a.xl = bf.xl;
        a.xg = bf.xg;
    }
    a.accumulate = accumulate;
    a.order = (c->opt[OPT_SPMM_ORDER] >= 2 || (c->opt[OPT_SPMM_ORDER] == 1 && A.skew)) ? A.order : nullptr;
    // GAT rewrites forwardAdj's values (the record is recognised by identity: A is a reference into c->adj, never a copy)
    const bool static_vals = val == A.val && !(c->gnn == DORY_GAT && &A == &c->adj[ADJ_IN]);
    const bool layouts = (static_vals || row_scale) && c->N > 0 && a.ld >= 32;   // K1s / K1b gather through copies of the static adjacency
    int rc = SPMM_NOT_MINE;
    if (layouts && c->opt[OPT_SPMM_VARIANT] == 2) rc = spmm_k1s(c, A, a, row_scale, bf);
    if (rc == SPMM_NOT_MINE && layouts && c->opt[OPT_SPMM_VARIANT] >= 1 && !bf16) rc = spmm_k1b(c, A, a, row_scale);
    if (rc == SPMM_NOT_MINE) rc = spmm_k1(c, A, a, bf);
    if (bf_out) *bf_out = bf;
    return rc;
}

// ---------------------------------------------------------------------------------------
// The bodies of dory_aggregate, one per model.  They run under its lock; a missing tensor is reported under its name.
#define AGG_NEED(ptr, l, nm) NEED_IN("dory_aggregate", ptr, l, nm)

// Engine::aggregateGCN (gcn_ops.cpp:130-191)
static int aggregate_gcn(dory_ctx *c, uint32_t layer, int dir) {
    Adjacency &In = c->adj[ADJ_IN], &Out = c->adj[ADJ_OUT];
    // opt-in "gcn_bf16_gather" (no reference counterpart): 1 = the forward aggregations read bf16 rows, 2 = the backward
    // ones too (spmm(): fp32 sums, same order).  K1b has no bf16 form: an explicit spmm_variant = 1 is refused
    const int64_t bfm = c->opt[OPT_GCN_BF16_GATHER];
    if (bfm && c->opt[OPT_SPMM_VARIANT] == 1)
        return fail(c, DORY_ERR_ARG, "aggregate: gcn_bf16_gather = %lld with spmm_variant = 1 (K1b has no bf16 form: spmm_variant 0 or 2)",
                    (long long)bfm);
    const bool bf_fwd = bfm >= 1, bf_bwd = bfm >= 2;
    if (dir == DORY_FORWARD) {
        if (layer >= c->L) return fail(c, DORY_ERR_ARG, "aggregate: layer %u out of range", layer);
        Tensor *in = layer == 0 ? find(c, 0, "x") : find(c, layer - 1, "h");
        AGG_NEED(fg, layer, "fg");
        AGG_NEED(ah, layer, "ah");
        if (!in) return fail(c, DORY_ERR_ARG, "aggregate: input tensor missing");
        if (tf_layer(c, layer)) {   // z_l = A (in_l W_l): gather d[l+1]-wide
            AGG_NEED(xw, layer, "xw"); AGG_NEED(fgxw, layer, "fgxw"); AGG_NEED(z, layer, "z");
            if (layer == 0) {   // the input and its ghost rows are static: transform both here
                Tensor &W = c->weights[0]["w"];
                int rc = gemm(c, 0, 0, c->N, c->dims[1], c->dims[0], *in, W, *xw);
                if (!rc && In.ghosts) rc = ghost_fp32_current(c, fg);   // (dory_halo_bf16_ghosts: the GEMM reads fp32 rows; fg@0 has no twin today)
                if (!rc && In.ghosts) rc = gemm(c, 0, 0, In.ghosts, c->dims[1], c->dims[0], *fg, W, *fgxw);
                if (rc) return rc;
            }   // deeper layers: apply_vertex(l-1) left xw@l, the forward exchange of layer l its ghost rows
            return spmm(c, In, In.val, 1, *xw, fgxw, *z, c->dims[layer + 1], 0, nullptr, bf_fwd);
        }
        // Opt-in "gcn_cache_ah0" (no reference counterpart; the reference recomputes it every epoch and so does the
        // default here): in full-graph training ah@0 = A_hat [x ; fg@0] is a constant of the run -- x and fg@0 come
        // from files, the adjacency never changes -- and with 288 GB of HBM it can simply stay.  The aggregation of
        // layer 0 is skipped while nothing it reads has been written through this ABI since it was last computed.
        const bool cache = layer == 0 && c->opt[OPT_GCN_CACHE_AH0] && !c->capturing;
        if (cache && c->ah0_valid) { c->ah0_skips++; return DORY_OK; }
        if (layer == 0) c->ah0_valid = false;
        c->agg_static_ghosts = layer == 0;
        const int rc = spmm(c, In, In.val, 1, *in, fg, *ah, c->dims[layer], 0, nullptr, bf_fwd);
        c->agg_static_ghosts = false;
        if (cache) c->ah0_valid = rc == DORY_OK;
        return rc;
    }
    if (tf_layer(c, layer)) {   // u_l = A^T g_l (ghost rows of g_l: backward exchange of layer l); dW_l = in_l^T u_l
        AGG_NEED(g, layer, "g"); AGG_NEED(bgg, layer, "bgg"); AGG_NEED(u, layer, "u");
        Tensor *in = layer == 0 ? find(c, 0, "x") : find(c, layer - 1, "h");
        if (!in) return fail(c, DORY_ERR_ARG, "aggregate: input tensor missing");
        const uint32_t Fin = c->dims[layer], Fout = c->dims[layer + 1];
        int rc = spmm(c, Out, Out.val, 1, *g, bgg, *u, Fout, 0, nullptr, bf_bwd);
        if (rc) return rc;
        if ((rc = gemm(c, 1, 0, Fin, Fout, c->N, *in, *u, c->wgrads[layer]["w"]))) return rc;
        if (layer == 0) return DORY_OK;
        AGG_NEED(aTg, layer - 1, "aTg");   // the gradient handed down: A^T (g_l W_l^T) = u_l W_l^T
        return gemm(c, 0, 1, c->N, Fin, Fout, *u, c->weights[layer]["w"], *aTg);
    }
    if (layer == 0 || layer >= c->L) return fail(c, DORY_ERR_ARG, "aggregate backward: layer %u out of range", layer);
    AGG_NEED(grad, layer, "grad");
    AGG_NEED(bg, layer - 1, "bg");
    AGG_NEED(aTg, layer - 1, "aTg");
    return spmm(c, Out, Out.val, 1, *grad, bg, *aTg, c->dims[layer], 0, nullptr, bf_bwd);
}

// What the two edge passes of the multi-head GAT on the sweep skeleton do alike (forward: the layout of the in-edges; source side of
// the backward: of the out-edges).  plan() decides the wide form -- option gatmh_bf16_wide: bf16 rows of 128 floats or more, several
// heads of 16 / 32 / 64 features, are gathered eight features per lane on 16-lane groups (same bits; gat_mh_sweep.hip); everywhere else:
// as with 0 -- and sizes the launches.  run() makes them: the blocks of local rows, `between` (what has to land before a ghost row
// is read), then the ghost blocks on top of the first launch's sums; without ghost rows `between`, then all blocks at once.
struct GatmhSweep {
    const DerivedAdj *S = nullptr;
    SweepLaunch sw;
    int plan(dory_ctx *c, const DerivedAdj &layout, const SpmmArgs &sa /* N, ld: as in the caller's own sweep_supported test */, uint32_t K,
             uint32_t D, bool ghosts, int shl, int pass, bool bf16) {
        S = &layout;
        const bool wide = bf16 && c->opt[OPT_GATMH_BF16_WIDE] == 1 && gatmh_wide_applies(K, D, sa.ld) && sweep_supported(sa, layout, GATMH_WIDE_GROUP);
        const int group = wide ? GATMH_WIDE_GROUP : gatmh_sweep_group(sa.ld);
        sw = sweep_launch(c, layout, sa.ld, group, ghosts, wide ? GATMH_WIDE_ROWS : gatmh_sweep_rows(layout, group, shl, pass), bf16, wide);
        return sw.done ? (int)DORY_OK : fail(c, DORY_ERR_ARG, "multi-head GAT sweep: gate counters not allocated (preallocate)");
    }
    template <class Between, class Part>
    int run(Between between, Part part) const {
        int rc;
        if (sw.two && (rc = part(sw.part(0, S->nb_local, false)))) return rc;
        if ((rc = between())) return rc;
        return part(sw.two ? sw.part(S->nb_local, S->nb, true) : sw.part(0, S->nb, false));
    }
};

// dory_gatmh_row_gather_hub_split: what a pass (0 forward, 1 destination-side edge pass, 2 source side) of the row-gather family over
// adjacency A hands its launcher -- the adjacency's chunk plan (built here at first use) and scratch for the chunk states (the buffer only
// ever grows: what a later kernel of the call was promised stays).  hubs->plan.nchunks == 0 -- the switch off, or no row over the
// chunk size -- launches what it always launched.
static int gatmh_hubs_for(dory_ctx *c, Adjacency &A, int pass, uint32_t ld, uint32_t ldk, GatmhHubs *hubs) {
    *hubs = GatmhHubs{};
    if (!c->gatmh_hub_chunk) return DORY_OK;
    int rc = hub_plan_ensure(c, A);
    if (rc || !A.hub_rows.nchunks) return rc;
    const size_t need = (size_t)A.hub_rows.nchunks * gatmh_rows_hub_state_floats(pass, ld, ldk) * sizeof(float);
    if ((rc = ensure_scratch(c, need))) return rc;
    hubs->plan = A.hub_rows;
    hubs->chunk = A.hub_chunk;
    hubs->state = c->scratch;
    return DORY_OK;
}

// dory_gatmh_row_gather_overlap: the two row lists of a pass of the row-gather family over adjacency A -- `first`: the interior rows the
// hub plan does not cut (they read no ghost row: launched before the wait for the exchange), `rest`: all others -- or *split == false
// where either list would be empty (no ghost, every row boundary, N == 0), or the switch is off: the pass launches what it always launched.
// The plan is built here at first use (not while recording).
static int gatmh_rows_lists_for(dory_ctx *c, Adjacency &A, bool *split, GatmhRowList *first, GatmhRowList *rest) {
    *split = false;
    if (!c->gatmh_rows_overlap || !A.ghosts || !c->N) return DORY_OK;
    const int rc = interior_plan_ensure(c, A);
    if (rc || !A.rows_split || !A.rows_first || A.rows_first >= c->N) return rc;
    *first = GatmhRowList{A.rows_split, A.rows_first, false};
    *rest = GatmhRowList{A.rows_split + A.rows_first, c->N - A.rows_first, true};
    *split = true;
    return DORY_OK;
}

// dory_gatmh_row_gather_edge_split: whether a pass of the row-gather family over adjacency A (the forward: the in-edges; the source
// side: the out-edges) runs the carry kernels over A's local-first copy, built here at first use (not while recording).  Not taken: the
// switch off; no ghost, no vertex, no entry (nothing to split); a hub chunk plan with chunks -- counted, where `count` says this is the
// pass itself and not dory_apply_edge asking ahead of it
static int gatmh_carry_taken(dory_ctx *c, Adjacency &A, bool count, bool *taken) {
    *taken = false;
    if (!c->gatmh_edge_split || !A.ghosts || !c->N || !A.nnz) return DORY_OK;
    int rc;
    if (c->gatmh_hub_chunk) {
        if ((rc = hub_plan_ensure(c, A))) return rc;
        if (A.hub_rows.nchunks) { if (count) c->gatmh_es_hub_fallbacks++; return DORY_OK; }
    }
    if ((rc = rows_edge_ensure(c, A))) return rc;
    *taken = A.rows_edge.built && A.rows_edge.idx && A.rows_edge.mid;
    return DORY_OK;
}
// ... and what such a pass (0 forward, 2 source side) hands its launcher: the copy and one state slot per row in the context's buffer
static int gatmh_carry_for(dory_ctx *c, Adjacency &A, int pass, uint32_t ld, uint32_t ldk, bool *taken, GatmhCarry *cy) {
    int rc = gatmh_carry_taken(c, A, true, taken);
    if (rc || !*taken) return rc;
    if ((rc = carry_state_ensure(c, (size_t)c->N * gatmh_rows_hub_state_floats(pass, ld, ldk) * sizeof(float)))) return rc;
    const RowsEdgeSplit &R = A.rows_edge;
    *cy = GatmhCarry{R.idx, R.mid, R.brows, R.nbrows, c->gatmh_carry_state};
    return DORY_OK;
}

// dory_gatmh_row_gather_bf16_wide: what a pass of the row-gather family hands its launcher -- fp32 rows, the shadow rows, or (the switch
// on, a shape of the wide form, 16-byte aligned shadow rows and twins) the shadow rows gathered 16 bytes a lane.  The wide form gives the
// narrow form's bits: nothing else of the schedule asks which of the two ran.  bf: after begin() -- the ghost rows' base (shadow rows
// or twin) is fixed there, before any of them has landed
static int gatmh_rows_gather_form(dory_ctx *c, bool bf16, uint32_t K, uint32_t D, uint32_t ld, const Bf16Rows &bf) {
    if (!bf16) return GATMH_ROWS_FP32;
    return c->gatmh_rows_wide && gatmh_rows_wide_ok(K, D, ld, bf.xl, bf.xg) ? GATMH_ROWS_BF16_WIDE : GATMH_ROWS_BF16;
}
// a bf16 pass of the family has run: it was wide, or narrow with the switch on
static void gatmh_rows_wide_count(dory_ctx *c, int form, uint64_t *wide) {
    if (form == GATMH_ROWS_BF16_WIDE) ++*wide;
    else if (c->gatmh_rows_wide) c->gatmh_rows8_narrow++;
}

// The multi-head GAT extension: edge softmax + weighted sum.
// opt-in "gatmh_bf16_gather" (no reference counterpart): 1 = the forward edge pass gathers the rows of z / fg_z rounded to
// bf16, 2 = the backward's source-side pass gathers do / bg_do likewise; scores, statistics, sums and outputs stay fp32.
// The sweep forms have bf16 kernels, and -- with dory_gatmh_row_gather_bf16 -- the row-gather family: where the dispatch below would
// take any other form the call is refused, never run in fp32
// opt-in "gatmh_bf16_wide" on top of it: where a pass runs on bf16 rows of 128 floats or more with several heads of 16 / 32 / 64
// features, its gathers fetch eight features per lane (16 bytes) on 16-lane groups -- the narrow bf16 form's bits
// which family the forward of a layer takes (aggregate_gatmh_forward's dispatch; dory_apply_edge asks ahead of it, for
// dory_gatmh_row_gather_overlap): the sweep form, the blocked form, else -- rows_forced or a partitioned run -- the row-gather family
struct GatmhFwdForm {
    bool rows_forced, blocked, sweep;
    int shl;
};
static GatmhFwdForm gatmh_fwd_form(dory_ctx *c, const Tensor *z, const Tensor *op, const Tensor *dpos, uint32_t K, uint32_t D) {
    Adjacency &In = c->adj[ADJ_IN];
    GatmhFwdForm f;
    const BlockedAdj &Bf = gatmh_blocked_for(In, z->ld);
    // dory_gatmh_row_gather = 1: the row-gather family (gat_mh_rows.hip) in place of every other; 0: where a partitioned call
    // finds neither layout below
    f.rows_forced = sw_value(c, SW_GATMH_ROW_GATHER) == 1;
    f.blocked = !f.rows_forced && c->opt[OPT_GATMH_BLOCKED] && In.blk.built && !In.blk.na && Bf.nb > 0 &&
                (D % 4 == 0 || K == 1) &&
                (size_t)Bf.nb * c->N * z->ld * sizeof(float) <= c->partial_bytes;
    const DerivedAdj &Sf = In.swp;
    f.shl = gatmh_sweep_hl(K, D, z->ld);
    // (the same addressing test the launchers make -- 32-bit byte offsets through the buffer resource -- so that a
    // partition they would refuse takes the blocked kernels instead of failing, as spmm() does)
    SpmmArgs sa{};
    sa.N = c->N; sa.ld = z->ld;
    f.sweep = !f.rows_forced && c->opt[OPT_GATMH_SWEEP] && c->opt[OPT_SPMM_VARIANT] == 2 && Sf.built && !Sf.na && Sf.nb > 0 &&
              f.shl != 0 && op && dpos && sweep_supported(sa, Sf, gatmh_sweep_group(z->ld));
    return f;
}

// the scores of the ghost sources of layer l0 from their exchanged z rows (dory_apply_edge; el is all the in-edge side needs)
static int gatmh_ghost_scores(dory_ctx *c, uint32_t l0) {
    const uint32_t K = c->heads[l0];
    NEED(z, l0, "z"); NEED(fgz, l0, "fg_z"); NEED(fgel, l0, "fg_el"); NEED(fger, l0, "fg_er");
    // dory_gatmh_bf16_ghosts: the exchange left the rows in fg_z's twin alone -- the scores come from the twin, the bits the fp32
    // kernel gives on the widened rows (the contract of dory_gatmh_halo_bf16: fg_el from rounded rows); nothing is widened
    if (fgz->twin && fgz->twin_state == DORY_GHOST_TWIN) {
        HIPCK(c, launch_gatmh_scores_bf16(c->adj[ADJ_IN].ghosts, K, z->cols / K, fgz->twin, fgz->ld, c->weights[l0]["a_l"].d,
                                          c->weights[l0]["a_r"].d, fgel->d, fger->d, fgel->ld, c->compute));
        if (!c->capturing) c->count[CNT_GATMH_TWIN_SCORES]++;
        return DORY_OK;
    }
    HIPCK(c, launch_gatmh_scores(c->adj[ADJ_IN].ghosts, K, z->cols / K, fgz->d, fgz->ld, c->weights[l0]["a_l"].d,
                                 c->weights[l0]["a_r"].d, fgel->d, fger->d, fgel->ld, c->compute));
    return DORY_OK;
}
// dory_gatmh_row_gather_overlap: dory_apply_edge left the ghost sources' scores of a layer to the moment the exchange of z has landed
// (wait_halo calls this once the compute stream waits for the ghost rows: every reader of fg_el / fg_er calls wait_halo first)
int gatmh_ghost_scores_flush(dory_ctx *c) {
    const int l0 = c->gatmh_scores_pending;
    c->gatmh_scores_pending = -1;
    if (l0 < 0) return DORY_OK;
    Timed t(c, "edge", c->compute);
    return gatmh_ghost_scores(c, (uint32_t)l0);
}

static int aggregate_gatmh_forward(dory_ctx *c, uint32_t fl) {
    Adjacency &In = c->adj[ADJ_IN];
    const uint32_t K = c->heads[fl];
    AGG_NEED(z, fl, "z"); AGG_NEED(el, fl, "el"); AGG_NEED(er, fl, "er"); AGG_NEED(m, fl, "m"); AGG_NEED(den, fl, "den"); AGG_NEED(o, fl, "o");
    const uint32_t D = z->cols / K;
    const int64_t bfm = c->opt[OPT_GATMH_BF16_GATHER];
    if (c->N == 0) {   // a rank without vertices: no row to aggregate, whatever the forms and options -- its (empty) exchange is finished as by any consumer
        if (fl < c->gatmh_fwd_swept.size()) c->gatmh_fwd_swept[fl] = 0;
        if (fl < c->gatmh_fwd_rows_bf16.size()) c->gatmh_fwd_rows_bf16[fl] = 0;
        return wait_halo(c);
    }
    {
        Timed t(c, "spmm", c->compute);
        const BlockedAdj &Bf = gatmh_blocked_for(In, z->ld);
        AGG_NEED(fgz, fl, "fg_z"); AGG_NEED(fgel, fl, "fg_el");
        const DerivedAdj &Sf = In.swp;
        Tensor *op = find(c, fl, "op"), *dpos = find(c, fl, "dpos");
        SpmmArgs sa{};
        sa.N = c->N; sa.ld = z->ld;
        const GatmhFwdForm form = gatmh_fwd_form(c, z, op, dpos, K, D);
        const bool rows_forced = form.rows_forced, blocked = form.blocked, sweep = form.sweep;
        const int shl = form.shl;
        // (dory_gatmh_row_gather_overlap: ghost scores dory_apply_edge left for the row-gather family, which this call does not take after all)
        if (c->gatmh_scores_pending >= 0 && (sweep || blocked || !(rows_forced || c->numNodes > 1))) { int wrc = wait_halo(c); if (wrc) return wrc; }
        const bool bf16 = bfm >= 1;
        // dory_gatmh_row_gather_bf16: where this call takes the row-gather family below, its bf16 form runs instead of the refusal
        const bool rows_bf16 = bf16 && sw_on(c, SW_GATMH_ROW_GATHER_BF16) && !sweep && !blocked && (rows_forced || c->numNodes > 1);
        if (c->gatmh_fwd_rows_bf16.size() < c->L) c->gatmh_fwd_rows_bf16.resize(c->L, 0);
        if (bf16 && !sweep && !rows_bf16)
            return fail(c, DORY_ERR_ARG, "aggregate: gatmh_bf16_gather = %lld needs the sweep form of the forward pass, which this call would not take: %s",
                        (long long)bfm,
                        rows_forced ? "dory_gatmh_row_gather = 1 (the row-gather kernels have no bf16 form)" :
                        !c->opt[OPT_GATMH_SWEEP] ? "gatmh_sweep = 0" :
                        c->opt[OPT_SPMM_VARIANT] != 2 ? "spmm_variant is not 2" :
                        !shl ? "heads x features outside the shapes of gatmh_sweep_hl" :
                        (!op || !dpos) ? "tensors op / dpos missing" : "the sweep layout of the in-edges does not apply to this graph");
        if (fl < c->gatmh_fwd_swept.size()) c->gatmh_fwd_swept[fl] = 0;
        c->gatmh_fwd_rows_bf16[fl] = 0;   // (set by the row-gather family's bf16 form alone)
        if (sweep) {
            // K1s's skeleton: sums in registers over all source blocks, single-pass softmax against the upper-bound shift
            int rc = ensure_scratch(c, gatmh_sweep_scratch_bytes(Sf, c->N, z->ld, el->ld));
            if (rc) return rc;
            GatmhSweep gs;
            if ((rc = gs.plan(c, Sf, sa, K, D, In.ghosts > 0, shl, 0, bf16))) return rc;
            // the rows the sweep gathers: z / fg_z, or (bf16) their rounded copies in the shadow buffer -- the local rows
            // converted now, the ghost rows once their exchange has landed
            Bf16Rows bf;
            if (bf16) {
                if ((rc = bf.begin(c, *z, fgz, In.ghosts, "gatmh_bf16_gather"))) return rc;
                c->gatmh_bf16_gathers_fwd++;
                if (gs.sw.wide) c->gatmh_bf16_gathers_fwd_wide++;
                if (bf.from_twin && !c->capturing) c->count[CNT_GATMH_TWIN_READS_SWEEP]++;
            }
            // dory_gatmh_bf16_ghosts: the fp32 form gathers fg_z's fp32 rows (the option was lowered after the exchange): widened first
            else if (In.ghosts && (rc = ghost_fp32_current(c, fgz))) return rc;
            const float *zs = bf16 ? bf.xl : z->d, *zgs = bf16 ? bf.xg : (In.ghosts ? fgz->d : nullptr), *a_l = c->weights[fl]["a_l"].d;
            HIPCK(c, launch_gatmh_sweep_begin(c->N, In.ghosts, K, z->ld, el->ld, Sf, el->d, fgel->d, c->scratch, c->compute));
            rc = gs.run([&]() -> int { const int r = wait_halo(c); return r ? r : bf.ghosts_landed(); }, [&](const SweepPart &p) -> int {
                HIPCK(c, launch_gatmh_forward_sweep_part(c->N, K, D, z->ld, el->ld, Sf, zs, zgs, er->d, a_l, o->d, op->d, c->scratch, p, el->d, fgel->d));
                return DORY_OK;
            });
            if (rc) return rc;
            // (dory_gatmh_bf16_ghosts: the finish / redo kernels read fg_z's fp32 rows -- a twin that alone is current is widened for them:
            //  correct, not a gain; twin-reading forms of these kernels are not built)
            if (In.ghosts && (rc = ghost_fp32_current(c, fgz))) return rc;
            HIPCK(c, launch_gatmh_forward_sweep_finish(c->N, K, D, z->ld, el->ld, In.ptr, In.idx, Sf, z->d, fgz->d, el->d, fgel->d,
                                                       er->d, o->d, op->d, m->d, den->d, dpos->d, c->scratch, c->compute, bf16));
            if (fl < c->gatmh_fwd_swept.size()) c->gatmh_fwd_swept[fl] = 1;
        }
        else if (blocked) {
            // "gatmh_fused_stats" (default 1): the blocks' own online softmax + a merge in the reduce kernel instead
            // of a statistics pass over all edges first; the blocks' (m_b, den_b) live in the scratch buffer
            float *stat_partial = nullptr;
            if (c->opt[OPT_GATMH_FUSED_STATS]) {
                int rc = ensure_scratch(c, (size_t)2 * Bf.nb * c->N * el->ld * sizeof(float));
                if (rc) return rc;
                stat_partial = c->scratch;
            }
            if (In.ghosts) { int grc = ghost_fp32_current(c, fgz); if (grc) return grc; }   // (dory_gatmh_bf16_ghosts: a reader of fp32 rows)
            HIPCK(c, launch_gatmh_forward_blocked(c->N, K, D, z->ld, el->ld, In.ptr, In.idx, Bf, z->d,
                                                  fgz->d, el->d, fgel->d, er->d, o->d, m->d, den->d, c->partial,
                                                  In.ghosts > 0, c->compute, stat_partial,
                                                  c->opt[OPT_GATMH_EL_ON_THE_FLY] ? c->weights[fl]["a_l"].d : nullptr));
        }
        else if (rows_forced || c->numNodes > 1) {
            // the row-gather family: the ghost rows have to have landed -- except, with dory_gatmh_row_gather_overlap, for the interior rows
            if (!op || !dpos || !gatmh_rows_ok(K, D, z->ld))
                return fail(c, DORY_ERR_ARG, "multi-head GAT: the row-gather kernels need op / dpos and K*D <= ld <= 256 (K = %u, D = %u, ld = %u)", K, D, z->ld);
            // bf16 form: z / fg_z from the shadow rows -- the local rows converted now, the ghost rows once their exchange has landed
            Bf16Rows bf;
            // dory_gatmh_row_gather_overlap: the interior rows (z / the local shadow rows alone) first, beside the exchange if one is in
            // flight; then the wait, the ghost rows' conversion or widening, and the rest -- around_halo's schedule, the same arithmetic
            // with and without an exchange in flight
            bool split;
            GatmhRowList first, rest;
            int rc = gatmh_rows_lists_for(c, In, &split, &first, &rest);
            if (rc) return rc;
            GatmhHubs hubs;   // dory_gatmh_row_gather_hub_split: the hub rows of the in-edges, if any
            if ((rc = gatmh_hubs_for(c, In, 0, z->ld, el->ld, &hubs))) return rc;
            // dory_gatmh_row_gather_edge_split: every row's local entries and self edge first -- beside the exchange, if one is in flight,
            // the boundary rows' states parked --, the wait, then the ghost entries; with nothing in flight (value 1) one launch of the
            // same kernel.  Where it takes the pass it decides it: no row lists
            bool carry;
            GatmhCarry cy;
            if ((rc = gatmh_carry_for(c, In, 0, z->ld, el->ld, &carry, &cy))) return rc;
            if (carry) split = false;
            if (rows_bf16 && (rc = bf.begin(c, *z, fgz, In.ghosts, "gatmh_bf16_gather"))) return rc;
            const float *a_l = c->weights[fl]["a_l"].d;
            const bool in_flight = c->halo_pending;
            const bool carry_two = carry && (c->gatmh_edge_split == 2 || in_flight);
            const int rform = carry ? (rows_bf16 ? GATMH_ROWS_BF16 : GATMH_ROWS_FP32) : gatmh_rows_gather_form(c, rows_bf16, K, D, z->ld, bf);
            auto launch_carry = [&](int walk) -> int {
                HIPCK(c, launch_gatmh_rows_forward_carry(c->N, K, D, z->ld, el->ld, In.ptr, rows_bf16 ? bf.xl : z->d, rows_bf16 ? bf.xg : fgz->d,
                                                         el->d, fgel->d, er->d, a_l, o->d, op->d, m->d, den->d, dpos->d, c->compute, rform, cy, walk));
                return DORY_OK;
            };
            auto launch = [&](const GatmhHubs *h, const GatmhRowList *rows) -> int {
                HIPCK(c, launch_gatmh_rows_forward(c->N, K, D, z->ld, el->ld, In.ptr, In.idx, rows_bf16 ? bf.xl : z->d,
                                                   rows_bf16 ? bf.xg : (In.ghosts ? fgz->d : nullptr), el->d, In.ghosts ? fgel->d : nullptr, er->d,
                                                   a_l, o->d, op->d, m->d, den->d, dpos->d, c->compute, rform, h, rows));
                return DORY_OK;
            };
            if (carry)
                rc = around_halo(c, carry_two, rows_bf16 ? &bf : nullptr, [&]() -> int { return launch_carry(GATMH_WALK_FIRST); }, [&]() -> int {
                    const int r = !rows_bf16 ? ghost_fp32_current(c, fgz) : (int)DORY_OK;
                    return r ? r : launch_carry(carry_two ? GATMH_WALK_SECOND : GATMH_WALK_BOTH);
                });
            else
            rc = around_halo(c, split, rows_bf16 ? &bf : nullptr, [&]() -> int { return launch(&hubs, &first); }, [&]() -> int {
                // (ghost_fp32_current waits for the exchange itself: after the interior launch)
                const int r = !rows_bf16 && In.ghosts ? ghost_fp32_current(c, fgz) : (int)DORY_OK;
                return r ? r : launch(&hubs, split ? &rest : nullptr);
            });
            if (rc) return rc;
            if (bf.from_twin && !c->capturing) c->count[CNT_GATMH_TWIN_READS_ROWS]++;
            if (split) { c->gatmh_ovl_fwd++; if (in_flight) c->gatmh_ovl_fwd_flight++; }
            if (carry) {
                c->gatmh_es_fwd++;
                if (carry_two && in_flight) c->gatmh_es_fwd_flight++;
                if (rows_bf16 && c->gatmh_rows_wide) c->gatmh_es_wide_not_taken++;
            }
            if (hubs.plan.nchunks) c->gatmh_hub_fwd++;
            if (fl < c->gatmh_fwd_swept.size()) c->gatmh_fwd_swept[fl] = 1;
            c->count[CNT_GATMH_ROWS_FWD]++;
            if (rows_bf16) {
                c->gatmh_fwd_rows_bf16[fl] = 1;
                c->gatmh_bf16_gathers_fwd++;
                c->count[CNT_GATMH_ROWS_BF16_FWD]++;
                gatmh_rows_wide_count(c, rform, &c->gatmh_rows8_fwd);
            }
        }
        else
            HIPCK(c, launch_gatmh_forward(c->N, K, D, z->ld, el->ld, In.ptr, In.idx, z->d, el->d, er->d,
                                          o->d, m->d, den->d, c->compute));
    }
    Timed t(c, "loss", c->compute);
    if (fl != c->L - 1) {
        AGG_NEED(hn, fl + 1, "h");
        HIPCK(c, launch_gatmh_elu(c->N, o->cols, o->d, o->ld, hn->d, hn->ld, c->compute));
    } else {
        AGG_NEED(lg, fl, "logits");
        HIPCK(c, launch_gatmh_head_mean(c->N, K, lg->cols, o->d, o->ld, lg->d, lg->ld, c->compute));
    }
    return DORY_OK;
}

// what the forms of the 8-head backward share
struct GatmhBwd {
    uint32_t fl, K, D;
    int64_t phase;   // option gatmh_bwd_phase: 0 = whole sweep; 1 / 2 = one phase (the caller moves the ghost rows)
    Tensor *z, *el, *er, *m, *den, *o, *dO, *dz, *tt, *del, *der, *st, *fgz, *fgel, *bgdo, *bgst;
};

// ghost destinations of the out-edges: their dO and st rows, between the two phases of a whole backward pass -- two exchanges, or
// (dory_gatmh_bwd_merged_exchange) one of merged rows, which `producer_packed` says the destination side has written already
// defer_last (dory_gatmh_row_gather_overlap; the row-gather family alone): the last exchange of the pass is issued deferred where
// halo_overlap allows -- the caller launches what reads no ghost row, then calls wait_halo before anything else
static int gatmh_backward_exchange(dory_ctx *c, const GatmhBwd &T, bool producer_packed = false, bool defer_last = false) {
    if (T.phase != 0 || c->numNodes <= 1) return DORY_OK;
    return gatmh_bwd_exchange(c, T.dO, T.bgdo, T.st, T.bgst, producer_packed, defer_last);
}

// The sweep forms (gat_mh_sweep.hip).  Destination side: this layer's forward ran on the skeleton and left the positive-branch
// sums, so t / der / st come from a row-wise kernel -- no edge pass.  Source side: the sweep over the out-edges' layout.
static int gatmh_backward_sweep(dory_ctx *c, const GatmhBwd &T, Tensor *op, Tensor *dpos, int shl, const SpmmArgs &sa, bool bf16) {
    Adjacency &Out = c->adj[ADJ_OUT];
    const DerivedAdj &So = Out.swp;
    const uint32_t K = T.K, D = T.D, ld = T.z->ld, ldk = T.el->ld, lds4 = T.st->ld / 4;
    float4 *st4 = reinterpret_cast<float4 *>(T.st->d);
    int rc;
    // dory_gatmh_bwd_merged_exchange: the send form writes the merged rows the exchange below ships (phase 0 only: asked in front of the launch)
    GatmhSend sd{};
    bool send = false, send16 = false;   // (send16, dory_gatmh_halo_bf16: the wire of this call ships do as bf16)
    if (T.phase == 0 && c->numNodes > 1 && (rc = gatmh_bwd_send_target(c, T.dO, T.st, &sd, &send, &send16))) return rc;
    if (T.phase != 2) {
        Timed t(c, "loss", c->compute);
        if (send)
            HIPCK(c, launch_gatmh_dst_rowwise_send(c->N, K, D, ld, ldk, T.dO->d, T.o->d, op->d, dpos->d, T.er->d, T.m->d, T.den->d, T.tt->d, T.der->d,
                                                   st4, lds4, sd, c->compute, send16));
        else
            HIPCK(c, launch_gatmh_dst_rowwise(c->N, K, D, ld, ldk, T.dO->d, T.o->d, op->d, dpos->d, T.er->d, T.m->d, T.den->d, T.tt->d, T.der->d,
                                              st4, lds4, c->compute));
    }
    if (T.phase == 1) return DORY_OK;
    if ((rc = gatmh_backward_exchange(c, T, send))) return rc;
    if ((rc = ensure_scratch(c, gatmh_src_sweep_scratch_bytes(So, c->N, Out.ghosts, K, ld, ldk)))) return rc;
    GatmhSweep gs;
    if ((rc = gs.plan(c, So, sa, K, D, Out.ghosts > 0, shl, 1, bf16))) return rc;
    {
        Timed t(c, "spmm", c->compute);
        // the rows the sweep gathers: do / bg_do, or (bf16) their rounded copies -- the ghost rows have landed by now
        // (phase 0: exchange_rows above made the compute stream wait; phase 2: the caller moved them before this call)
        Bf16Rows bf;
        if (bf16) {
            if ((rc = bf.begin(c, *T.dO, T.bgdo, Out.ghosts, "gatmh_bf16_gather")) || (rc = bf.ghosts_landed())) return rc;
            c->gatmh_bf16_gathers_src++;
            if (gs.sw.wide) c->gatmh_bf16_gathers_src_wide++;
            if (bf.from_twin && !c->capturing) c->count[CNT_GATMH_TWIN_READS_SWEEP]++;
        }
        // dory_gatmh_bf16_ghosts: the fp32 form gathers bg_do's fp32 rows (gatmh_bwd_phase = 2 with the option lowered since the rows landed)
        else if (Out.ghosts && (rc = ghost_fp32_current(c, T.bgdo))) return rc;
        const float *dos = bf16 ? bf.xl : T.dO->d, *dogs = bf16 ? bf.xg : (Out.ghosts ? T.bgdo->d : nullptr);
        HIPCK(c, launch_gatmh_src_sweep_begin(c->N, Out.ghosts, K, ld, ldk, So, st4, reinterpret_cast<const float4 *>(T.bgst->d), lds4,
                                              c->scratch, c->compute));
        rc = gs.run([] { return (int)DORY_OK; }, [&](const SweepPart &p) -> int {
            HIPCK(c, launch_gatmh_src_sweep_part(c->N, Out.ghosts, K, D, ld, ldk, So, dos, dogs, T.el->d, T.dz->d, c->scratch, p));
            return DORY_OK;
        });
        if (rc) return rc;
        HIPCK(c, launch_gatmh_src_sweep_finish(c->N, K, D, ld, ldk, So, T.z->d, T.el->d, T.dO->d, T.der->d, c->weights[T.fl]["a_l"].d,
                                               c->weights[T.fl]["a_r"].d, T.del->d, T.dz->d, c->scratch, c->compute, bf16));
    }
    // (the attention gradients' column sums take the scratch buffer next: the sweep's sums are consumed by then)
    if ((rc = ensure_scratch(c, (size_t)2048 * T.z->cols * sizeof(float) + 256))) return rc;
    HIPCK(c, launch_gatmh_dattn(c->N, K, D, ld, ldk, T.z->d, T.del->d, T.der->d, c->wgrads[T.fl]["a_l"].d,
                                c->wgrads[T.fl]["a_r"].d, c->scratch, c->scratch_bytes, c->compute));
    return DORY_OK;
}

// the source-blocked form (gat_mh_blocked.hip): destination side over the in-edges' blocks, source side over the out-edges'
static int gatmh_backward_blocked(dory_ctx *c, const GatmhBwd &T, const BlockedAdj &Bbi, const BlockedAdj &Bbo) {
    const uint32_t K = T.K, D = T.D, ld = T.z->ld, ldk = T.el->ld, lds4 = T.st->ld / 4;
    float4 *st4 = reinterpret_cast<float4 *>(T.st->d);
    // (dory_gatmh_bf16_ghosts: both sides read fp32 rows -- fg_z here, bg_do after the exchange)
    if (T.phase != 2 && c->adj[ADJ_IN].ghosts) { int grc = ghost_fp32_current(c, T.fgz); if (grc) return grc; }
    if (T.phase != 2) {   // destination side: t, der, st
        Timed t(c, "spmm", c->compute);
        HIPCK(c, launch_gatmh_backward_blocked_dst(c->N, K, D, ld, ldk, Bbi, T.z->d, T.fgz->d, T.el->d, T.fgel->d,
                                                   T.er->d, T.m->d, T.den->d, T.dO->d, T.tt->d, T.der->d, c->partial, st4, lds4,
                                                   c->adj[ADJ_IN].ghosts > 0, c->compute,
                                                   // (el from the gathered row only where the forward formed its statistics that
                                                   //  way too: its ELFLY form needs the fused statistics -- same rounding of alpha)
                                                   (c->opt[OPT_GATMH_EL_ON_THE_FLY] && c->opt[OPT_GATMH_FUSED_STATS]) ? c->weights[T.fl]["a_l"].d : nullptr));
    }
    if (T.phase == 1) return DORY_OK;
    int rc = gatmh_backward_exchange(c, T);
    if (rc || (c->adj[ADJ_OUT].ghosts && (rc = ghost_fp32_current(c, T.bgdo)))) return rc;
    Timed t(c, "spmm", c->compute);
    HIPCK(c, launch_gatmh_backward_blocked_src(c->N, K, D, ld, ldk, Bbo, T.z->d, T.el->d, T.dO->d, T.bgdo->d, st4,
                                               reinterpret_cast<const float4 *>(T.bgst->d), lds4, T.der->d,
                                               c->weights[T.fl]["a_l"].d, c->weights[T.fl]["a_r"].d, T.del->d, T.dz->d,
                                               c->partial, c->adj[ADJ_OUT].ghosts > 0, c->compute));
    HIPCK(c, launch_gatmh_dattn(c->N, K, D, ld, ldk, T.z->d, T.del->d, T.der->d, c->wgrads[T.fl]["a_l"].d,
                                c->wgrads[T.fl]["a_r"].d, c->scratch, c->scratch_bytes, c->compute));
    return DORY_OK;
}

// the row-gather family (gat_mh_rows.hip), in the two phases of the blocked form: the destination side over the in-edges (ghost
// sources) -- the row-wise kernel on op / dpos where this layer's forward left them and it covers the shape (`rowwise`), else an edge
// pass --, the exchange of do / st (pack kernels: nothing here writes send rows), the source side over the out-edges (ghost destinations)
// dst_bf16 / src_bf16 (dory_gatmh_row_gather_bf16): the edge pass gathers z / fg_z, the source side do / bg_do, from the shadow rows
// (the caller has reserved them); the ghost rows have landed where either is converted -- fg_z since the forward, bg_do after the exchange
static int gatmh_backward_rows(dory_ctx *c, const GatmhBwd &T, Tensor *op, Tensor *dpos, bool rowwise, bool dst_bf16, bool src_bf16) {
    Adjacency &In = c->adj[ADJ_IN], &Out = c->adj[ADJ_OUT];
    const uint32_t K = T.K, D = T.D, ld = T.z->ld, ldk = T.el->ld, lds4 = T.st->ld / 4;
    float4 *st4 = reinterpret_cast<float4 *>(T.st->d);
    int rc;
    if (!gatmh_rows_ok(K, D, ld))
        return fail(c, DORY_ERR_ARG, "multi-head GAT: the row-gather kernels need K*D <= ld <= 256 (K = %u, D = %u, ld = %u)", K, D, ld);
    if (T.phase != 2) {   // destination side: t, der, st
        if (rowwise) {
            Timed t(c, "loss", c->compute);
            HIPCK(c, launch_gatmh_dst_rowwise(c->N, K, D, ld, ldk, T.dO->d, T.o->d, op->d, dpos->d, T.er->d, T.m->d, T.den->d, T.tt->d, T.der->d,
                                              st4, lds4, c->compute));
            c->count[CNT_GATMH_ROWS_DST_ROWWISE]++;
        } else {
            Timed t(c, "spmm", c->compute);
            Bf16Rows bf;
            if (dst_bf16 && ((rc = bf.begin(c, *T.z, T.fgz, In.ghosts, "gatmh_bf16_gather")) || (rc = bf.ghosts_landed()))) return rc;
            // (dory_gatmh_bf16_ghosts: the fp32 edge pass -- a layer whose forward swept, the option lowered since -- reads fg_z's fp32 rows)
            if (!dst_bf16 && In.ghosts && (rc = ghost_fp32_current(c, T.fgz))) return rc;
            if (bf.from_twin && !c->capturing) c->count[CNT_GATMH_TWIN_READS_ROWS]++;
            GatmhHubs hubs;   // dory_gatmh_row_gather_hub_split: the hub rows of the in-edges, if any
            if ((rc = gatmh_hubs_for(c, In, 1, ld, ldk, &hubs))) return rc;
            const int rform = gatmh_rows_gather_form(c, dst_bf16, K, D, ld, bf);
            HIPCK(c, launch_gatmh_rows_dst(c->N, K, D, ld, ldk, In.ptr, In.idx, dst_bf16 ? bf.xl : T.z->d,
                                           dst_bf16 ? bf.xg : (In.ghosts ? T.fgz->d : nullptr), T.el->d, In.ghosts ? T.fgel->d : nullptr, T.er->d,
                                           c->weights[T.fl]["a_l"].d, T.m->d, T.den->d, T.dO->d, T.tt->d, T.der->d, st4, lds4, c->compute, rform,
                                           &hubs));
            if (hubs.plan.nchunks) c->gatmh_hub_dst++;
            c->count[CNT_GATMH_ROWS_DST_EDGE]++;
            if (dst_bf16) { c->count[CNT_GATMH_ROWS_BF16_DST_EDGE]++; gatmh_rows_wide_count(c, rform, &c->gatmh_rows8_dst); }
        }
    }
    if (T.phase == 1) return DORY_OK;
    // dory_gatmh_row_gather_overlap: the interior sources (every destination local: do / st alone) run beside the pass's last exchange,
    // which is then issued deferred (halo_overlap); the wait, bg_do's conversion or widening and the rest follow.  Phase 2: the same two
    // launches with nothing in flight
    bool split;
    GatmhRowList first, rest;
    if ((rc = gatmh_rows_lists_for(c, Out, &split, &first, &rest))) return rc;
    // dory_gatmh_row_gather_edge_split: every source's local destinations and self edge beside that exchange, the ghost destinations
    // after the wait; it takes the deferral too, and where it takes the pass it decides it
    bool carry;
    GatmhCarry cy;
    if ((rc = gatmh_carry_for(c, Out, 2, ld, ldk, &carry, &cy))) return rc;
    if (carry) split = false;
    if ((rc = gatmh_backward_exchange(c, T, false, split || carry))) return rc;
    {
        Timed t(c, "spmm", c->compute);
        // (phase 0: the exchange above made the compute stream wait for bg_do, or around_halo does; phase 2: the caller moved it before this call)
        Bf16Rows bf;
        GatmhHubs hubs;   // dory_gatmh_row_gather_hub_split: the hub rows of the out-edges, if any (the merge has read the states before
        if ((rc = gatmh_hubs_for(c, Out, 2, ld, ldk, &hubs))) return rc;   //  launch_gatmh_dattn below takes the scratch: one stream)
        if (src_bf16 && (rc = bf.begin(c, *T.dO, T.bgdo, Out.ghosts, "gatmh_bf16_gather"))) return rc;
        const bool in_flight = c->halo_pending;
        const bool carry_two = carry && (c->gatmh_edge_split == 2 || in_flight);
        const int rform = carry ? (src_bf16 ? GATMH_ROWS_BF16 : GATMH_ROWS_FP32) : gatmh_rows_gather_form(c, src_bf16, K, D, ld, bf);
        auto launch_carry = [&](int walk) -> int {
            HIPCK(c, launch_gatmh_rows_src_carry(c->N, K, D, ld, ldk, Out.ptr, T.z->d, T.el->d, src_bf16 ? bf.xl : T.dO->d,
                                                 src_bf16 ? bf.xg : T.bgdo->d, st4, reinterpret_cast<const float4 *>(T.bgst->d), lds4, T.der->d,
                                                 c->weights[T.fl]["a_l"].d, c->weights[T.fl]["a_r"].d, T.del->d, T.dz->d, c->compute, rform, cy, walk));
            return DORY_OK;
        };
        auto launch = [&](const GatmhHubs *h, const GatmhRowList *rows) -> int {
            HIPCK(c, launch_gatmh_rows_src(c->N, K, D, ld, ldk, Out.ptr, Out.idx, T.z->d, T.el->d, src_bf16 ? bf.xl : T.dO->d,
                                           src_bf16 ? bf.xg : (Out.ghosts ? T.bgdo->d : nullptr), st4,
                                           Out.ghosts ? reinterpret_cast<const float4 *>(T.bgst->d) : nullptr, lds4, T.der->d,
                                           c->weights[T.fl]["a_l"].d, c->weights[T.fl]["a_r"].d, T.del->d, T.dz->d, c->compute, rform, h, rows));
            return DORY_OK;
        };
        if (carry)
            rc = around_halo(c, carry_two, src_bf16 ? &bf : nullptr, [&]() -> int { return launch_carry(GATMH_WALK_FIRST); }, [&]() -> int {
                const int r = !src_bf16 ? ghost_fp32_current(c, T.bgdo) : (int)DORY_OK;
                return r ? r : launch_carry(carry_two ? GATMH_WALK_SECOND : GATMH_WALK_BOTH);
            });
        else
        rc = around_halo(c, split, src_bf16 ? &bf : nullptr, [&]() -> int { return launch(&hubs, &first); }, [&]() -> int {
            const int r = !src_bf16 && Out.ghosts ? ghost_fp32_current(c, T.bgdo) : (int)DORY_OK;
            return r ? r : launch(&hubs, split ? &rest : nullptr);
        });
        if (rc) return rc;
        if (bf.from_twin && !c->capturing) c->count[CNT_GATMH_TWIN_READS_ROWS]++;
        if (split) { c->gatmh_ovl_src++; if (in_flight) c->gatmh_ovl_src_flight++; }
        if (carry) {
            c->gatmh_es_src++;
            if (carry_two && in_flight) c->gatmh_es_src_flight++;
            if (src_bf16 && c->gatmh_rows_wide) c->gatmh_es_wide_not_taken++;
        }
        if (hubs.plan.nchunks) c->gatmh_hub_src++;
        c->count[CNT_GATMH_ROWS_SRC]++;
        if (src_bf16) {
            c->gatmh_bf16_gathers_src++;
            c->count[CNT_GATMH_ROWS_BF16_SRC]++;
            gatmh_rows_wide_count(c, rform, &c->gatmh_rows8_src);
        }
    }
    HIPCK(c, launch_gatmh_dattn(c->N, K, D, ld, ldk, T.z->d, T.del->d, T.der->d, c->wgrads[T.fl]["a_l"].d,
                                c->wgrads[T.fl]["a_r"].d, c->scratch, c->scratch_bytes, c->compute));
    return DORY_OK;
}

// the backward of the edge softmax + weighted sum: the sweep forms, else the blocked kernels (same m / den / st semantics),
// else (partitioned runs; dory_gatmh_row_gather = 1: first) the row-gather family, else (single partition) the row-wise kernels
static int aggregate_gatmh_backward(dory_ctx *c, uint32_t fl) {
    Adjacency &In = c->adj[ADJ_IN], &Out = c->adj[ADJ_OUT];
    const uint32_t K = c->heads[fl];
    AGG_NEED(z, fl, "z"); AGG_NEED(el, fl, "el"); AGG_NEED(er, fl, "er"); AGG_NEED(m, fl, "m"); AGG_NEED(den, fl, "den"); AGG_NEED(o, fl, "o");
    AGG_NEED(dO, fl, "do"); AGG_NEED(dz, fl, "dz"); AGG_NEED(tt, fl, "t"); AGG_NEED(del, fl, "del"); AGG_NEED(der, fl, "der");
    AGG_NEED(st, fl, "st"); AGG_NEED(fgz, fl, "fg_z"); AGG_NEED(fgel, fl, "fg_el"); AGG_NEED(bgdo, fl, "bg_do"); AGG_NEED(bgst, fl, "bg_st");
    const uint32_t D = z->cols / K;
    const GatmhBwd T{fl, K, D, c->opt[OPT_GATMH_BWD_PHASE], z, el, er, m, den, o, dO, dz, tt, del, der, st, fgz, fgel, bgdo, bgst};
    const int64_t bfm = c->opt[OPT_GATMH_BF16_GATHER];
    if (c->N == 0) {   // a rank without vertices: its share of the attention gradients is zero, and it takes part in the sweep's exchange(s) of no rows
        for (const char *nm : {"a_l", "a_r"}) {
            Tensor &g = c->wgrads[fl][nm];
            HIPCK(c, hipMemsetAsync(g.d, 0, (size_t)g.rows * g.ld * sizeof(float), c->compute));
        }
        return gatmh_backward_exchange(c, T);
    }
    const int shl = gatmh_sweep_hl(K, D, z->ld);
    Tensor *op = find(c, fl, "op"), *dpos = find(c, fl, "dpos");
    const bool dst_rowwise = c->opt[OPT_GATMH_SWEEP] && shl && op && dpos && fl < c->gatmh_fwd_swept.size() && c->gatmh_fwd_swept[fl] &&
                             ((z->ld >> 2) % (uint32_t)shl) == 0;
    const DerivedAdj &So = Out.swp;
    SpmmArgs sa{};     // the launchers' addressing tests (rows and the 16-byte statistics records through buffer resources): a
    sa.N = c->N; sa.ld = z->ld;   // partition they would refuse takes the blocked kernels
    const bool src_sweep = c->opt[OPT_GATMH_SWEEP] && c->opt[OPT_SPMM_VARIANT] == 2 && shl && So.built && !So.na && So.nb > 0 &&
                           ((z->ld >> 2) % (uint32_t)shl) == 0 && sweep_supported(sa, So, gatmh_sweep_group(z->ld)) &&
                           (uint64_t)std::max(c->N, Out.ghosts) * K * 16u < (1ull << 32) && K * 16u < (1u << 24);
    // bf16 rows of do / bg_do for the source-side sweep (gatmh_bf16_gather = 2): refused, before anything is launched, where
    // the call would not take that sweep; the shadow buffer is sized here too (it cannot grow inside a recording)
    const bool bf16 = bfm >= 2;
    const bool rows_forced = sw_value(c, SW_GATMH_ROW_GATHER) == 1;
    const bool sweeps = !rows_forced && dst_rowwise && src_sweep;
    const BlockedAdj &Bbi = gatmh_blocked_for(In, z->ld), &Bbo = gatmh_blocked_for(Out, z->ld);
    const uint32_t nbmax = std::max(Bbi.nb, Bbo.nb);
    const bool blocked = !rows_forced && !sweeps && c->opt[OPT_GATMH_BLOCKED] && In.blk.built && Out.blk.built && !In.blk.na && !Out.blk.na &&
                         nbmax > 0 && gatmh_backward_blocked_ok(K, D, z->ld) &&
                         (size_t)nbmax * c->N * (z->ld + K) * sizeof(float) <= c->partial_bytes;
    // the row-gather family (op / dpos are current whichever family's forward left them; gatmh_sweep is not asked), and what of it
    // runs on bf16 rows with dory_gatmh_row_gather_bf16: the source side by the option; the destination side's edge pass where this
    // layer's forward ran the family's bf16 form -- its scores have to be the forward's scores
    const bool rows = !sweeps && !blocked && (rows_forced || c->numNodes > 1);
    const bool rows_dst_rowwise = shl && op && dpos && fl < c->gatmh_fwd_swept.size() && c->gatmh_fwd_swept[fl] && ((z->ld >> 2) % (uint32_t)shl) == 0;
    const bool rows_bf16 = rows && sw_on(c, SW_GATMH_ROW_GATHER_BF16);
    const bool rows_src_bf16 = rows_bf16 && bf16;
    const bool rows_dst_bf16 = rows_bf16 && !rows_dst_rowwise && fl < c->gatmh_fwd_rows_bf16.size() && c->gatmh_fwd_rows_bf16[fl];
    if (bf16 && !sweeps && !rows_src_bf16)
        return fail(c, DORY_ERR_ARG, "aggregate: gatmh_bf16_gather = 2 needs the sweep forms of the backward pass, which this call would not take: %s",
                    rows_forced ? "dory_gatmh_row_gather = 1 (the row-gather kernels have no bf16 form)" :
                    !c->opt[OPT_GATMH_SWEEP] ? "gatmh_sweep = 0" :
                    c->opt[OPT_SPMM_VARIANT] != 2 ? "spmm_variant is not 2" :
                    !shl ? "heads x features outside the shapes of gatmh_sweep_hl" :
                    !dst_rowwise ? "this layer's forward pass did not run the sweep form" : "the sweep layout of the out-edges does not apply to this graph");
    int rc;
    // dory_gatmh_bf16_ghosts: N rows only where the ghost rows will be read from a twin -- bg_do's once the exchange of this call has landed
    // them there (a whole pass), or as it stands now (phase 2: the caller has moved the rows); fg_z's as it stands since the forward
    const bool do_twin = T.phase == 0 ? gatmh_do_lands_in_twin(c, dO, bgdo) : bgdo->twin_current() && !bgdo->raw_handed;
    const bool z_twin = fgz->twin_current() && !fgz->raw_handed;
    if (bf16 && T.phase != 1 && (rc = bf16_reserve(c, (uint64_t)c->N + (do_twin ? 0 : Out.ghosts), z->ld, "gatmh_bf16_gather"))) return rc;
    if (rows_dst_bf16 && T.phase != 2 && (rc = bf16_reserve(c, (uint64_t)c->N + (z_twin ? 0 : In.ghosts), z->ld, "gatmh_bf16_gather"))) return rc;
    if (T.phase != 2) {
        Timed t(c, "loss", c->compute);
        if (fl == c->L - 1) {
            AGG_NEED(gr, fl, "grad");
            HIPCK(c, launch_gatmh_head_expand(c->N, K, gr->cols, gr->d, gr->ld, dO->d, dO->ld, c->compute));
        } else {
            AGG_NEED(dh, fl + 1, "dh");
            HIPCK(c, launch_gatmh_elu_bwd(c->N, o->cols, dh->d, dh->ld, o->d, o->ld, dO->d, dO->ld, c->compute));
        }
    }
    if ((rc = ensure_scratch(c, (size_t)2048 * z->cols * sizeof(float) + (size_t)c->N * K * 16 + 256))) return rc;
    if (sweeps) return gatmh_backward_sweep(c, T, op, dpos, shl, sa, bf16);
    if (blocked) return gatmh_backward_blocked(c, T, Bbi, Bbo);
    if (rows) return gatmh_backward_rows(c, T, op, dpos, rows_dst_rowwise, rows_dst_bf16, rows_src_bf16);
    Timed t(c, "spmm", c->compute);
    HIPCK(c, launch_gatmh_backward(c->N, K, D, z->ld, el->ld, In.ptr, In.idx, Out.ptr, Out.idx, z->d, el->d,
                                   er->d, m->d, den->d, dO->d, c->weights[fl]["a_l"].d, c->weights[fl]["a_r"].d,
                                   tt->d, del->d, der->d, dz->d, c->wgrads[fl]["a_l"].d, c->wgrads[fl]["a_r"].d,
                                   c->scratch, c->scratch_bytes, c->compute));
    return DORY_OK;
}

// dory_gat_bf16_gather: the shadow rows of the largest aggregation of the model -- (N + ghosts) rows of the widest z / grad --
// reserved at once (the setter, the first eager aggregation), so that an epoch recorded after one eager epoch finds nothing to grow
int gat_bf16_reserve_all(dory_ctx *c) {
    if (!c->prealloc || c->gnn != DORY_GAT || !c->gat_bf16_mode) return DORY_OK;
    uint32_t maxld = 0;
    for (uint32_t l = 0; l < c->L; ++l) maxld = std::max(maxld, pad_ld(c->dims[l + 1]));
    return bf16_reserve(c, (uint64_t)c->N + std::max(c->adj[ADJ_IN].ghosts, c->adj[ADJ_OUT].ghosts), maxld, "dory_gat_bf16_gather");
}

// Engine::aggregateGAT (gat_ops.cpp:173-243), the reference's prototype: edge scores that depend on the destination only
static int aggregate_gat(dory_ctx *c, uint32_t fl, int dir) {
    Adjacency &In = c->adj[ADJ_IN], &Out = c->adj[ADJ_OUT];
    const uint32_t F = c->dims[fl + 1];
    AGG_NEED(z, fl, "z");
    AGG_NEED(fgz, fl, "fg_z");
    // dory_apply_edge leaves, next to the per-edge tensors "A" / "dA", the one value all
    // edges of a destination share; while that is current the SpMM gathers unweighted
    // (K1b) and scales per row.  A caller that overwrote "A"/"dA" gets the general K1 path.
    // Round 6: with scores that depend on the destination only, BOTH in-edge aggregations of a layer -- the forward's
    // ah = z + arow (.) S and the backward's aTg += drow (.) S -- are row-scaled copies of ONE unweighted neighbour sum
    // S[v] = sum over in-edges of z[src] (ghosts included).  The forward computes S (tensor "nsum", same K1s launch(es), unit
    // weights), the backward reuses it: two aggregations per layer and epoch instead of three ("gat_reuse_nsum"; a caller who
    // replaced z / fg_z / "A" / "dA" in between gets the general path).
    Tensor *nsum = find(c, fl, "nsum"), *ones = find(c, 0, "ones");
    const bool reuse = c->opt[OPT_GAT_REUSE_NSUM] && nsum && ones && fl < c->gat_nsum_valid.size() && z->ld == nsum->ld;
    // opt-in dory_gat_bf16_gather (no reference counterpart): 1 = the aggregations that gather z / fg_z read them rounded to bf16
    // (the forward's, and the backward's dA-weighted term, reused or recomputed), 2 = the backward's A^T grad gather of grad / bg_d
    // too (spmm(): fp32 sums, same order).  K1b has no bf16 form: an explicit spmm_variant = 1 is refused
    const int bfm = c->gat_bf16_mode;
    if (bfm && c->opt[OPT_SPMM_VARIANT] == 1)
        return fail(c, DORY_ERR_ARG, "aggregate: dory_gat_bf16_gather mode %d with spmm_variant = 1 (K1b has no bf16 form: spmm_variant 0 or 2)", bfm);
    const bool bf_z = bfm >= 1, bf_grad = bfm >= 2;
    // the shadow buffer cannot grow inside a recording: all of it at the first eager aggregation, for the widest layer
    if (bfm && !c->capturing) { int rrc = gat_bf16_reserve_all(c); if (rrc) return rrc; }
    if (dir == DORY_FORWARD) {
        AGG_NEED(ah, fl, "ah");
        Tensor *arow = find(c, fl, "arow");
        const bool fast = arow && fl < c->gat_arow_valid.size() && c->gat_arow_valid[fl];
        if (fl < c->gat_nsum_valid.size()) c->gat_nsum_valid[fl] = 0;
        if (fast && reuse && c->N) {
            if (!c->gat_ones_set) {
                HIPCK(c, hipMemsetD32Async((hipDeviceptr_t)ones->d, 0x3f800000, c->N, c->compute));
                c->gat_ones_set = true;
            }
            Bf16Rows bf;
            int rc = spmm(c, In, In.val, 0, *z, fgz, *nsum, F, 0, ones->d, bf_z, &bf);
            if (rc) return rc;
            if (c->last_spmm_unit) {      // (K1 -- graphs without a blocked layout -- gathers with the per-edge values: not a unit sum)
                Timed t(c, "spmm", c->compute);
                // on bf16 rows the self row is the rounded one: the shadow buffer still holds z's rows, [0, N) x ld, as the launch(es)
                // above gathered them (nothing between here and there writes it: the combine kernel only reads it)
                if (bf.on()) HIPCK(c, launch_row_axpy_bf16(ah->d, nsum->d, arow->d, c->bf16_rows, c->N, z->ld, c->compute));
                else HIPCK(c, launch_row_axpy(ah->d, nsum->d, arow->d, z->d, c->N, z->ld, c->compute));
                c->gat_nsum_valid[fl] = 1;
                c->gat_nsum_bf16[fl] = bf.on() ? 1 : 0;
                return DORY_OK;
            }
            // (the K1 launch above counted as an aggregation on bf16 rows already; the general path below is a second one)
        }
        { int mrc = gat_materialize(c, fl, 2); if (mrc) return mrc; }   // (K1 reads the per-edge values)
        return spmm(c, In, In.val, 2, *z, fgz, *ah, F, 0, fast ? arow->d : nullptr, bf_z);
    }
    AGG_NEED(grad, fl, "grad");
    AGG_NEED(bgd, fl, "bg_d");
    AGG_NEED(dA, fl, "dA");
    AGG_NEED(aTg, fl, "aTg");
    // fresh two-term sum (the CUDA path's semantics, gat_ops.cpp:155-163): A^T.dP then += dA.Z
    int rc = spmm(c, Out, Out.val, 0, *grad, bgd, *aTg, F, 0, nullptr, bf_grad);
    if (rc) return rc;
    Tensor *drow = find(c, fl, "drow");
    const bool fast = drow && fl < c->gat_drow_valid.size() && c->gat_drow_valid[fl];
    // the kept neighbour sum serves only the rounding the mode asks for now (a mode switched between forward and backward: recompute)
    if (fast && reuse && c->gat_nsum_valid[fl] && (c->gat_nsum_bf16[fl] != 0) == bf_z) {
        Timed t(c, "spmm", c->compute);
        HIPCK(c, launch_row_axpy(aTg->d, nsum->d, drow->d, nullptr, c->N, aTg->ld, c->compute));
        return DORY_OK;
    }
    { int mrc = gat_materialize(c, fl, 4); if (mrc) return mrc; }
    return spmm(c, In, dA->d, 0, *z, fgz, *aTg, F, 1, fast ? drow->d : nullptr, bf_z);
}

#undef AGG_NEED

// dory_halo_fused_pack_rowwise: the row-wise kernel about to write `out` (N rows of `cols` columns) may store its rows into the send
// buffer too -- what gemm() (abi_context.hip) asks for a product, with the switch in front; the previous exchange has finished
// reading the buffer before true comes back.  A one-column tensor (ld == 1) is left to the pack kernels, whatever the wire.
static int rowwise_send_target(dory_ctx *c, const Tensor *out, uint32_t cols, GemmSend *sd, int *dir, bool *send) {
    *send = sw_on(c, SW_HALO_FUSED_PACK_ROWWISE) && out->cols == cols && (out->ld & 3u) == 0 && fused_pack_target(c, out, c->N, sd, dir);
    if (!*send) return DORY_OK;
    sd->which = 0;
    sd->cols = cols;
    return wait_halo(c);
}
// ... and after its launch: the rows are in the buffer (stamped), or the plain kernel ran after all
static void rowwise_sent(dory_ctx *c, const Tensor *out, int dir, const GemmSend &sd, bool fused) {
    if (fused) fused_pack_stamp(c, out, dir, sd, true);
    else fused_note_write(c, out);
}

}  // namespace dory

using namespace dory;

extern "C" {

int dory_aggregate(dory_ctx *c, uint32_t layer, int dir) {
    CHECK_CTX(c);
    if (!c->prealloc) return fail(c, DORY_ERR_ARG, "aggregate: preallocate first");
    if (c->gnn == DORY_GCN) return aggregate_gcn(c, layer, dir);
    // Engine::aggregateGAT (gat_ops.cpp:173-243): tensors live at layer-1
    if (layer == 0 || layer > c->L) return fail(c, DORY_ERR_ARG, "aggregate GAT: layer %u out of range", layer);
    if (c->gnn != DORY_GATMH) return aggregate_gat(c, layer - 1, dir);
    return dir == DORY_FORWARD ? aggregate_gatmh_forward(c, layer - 1) : aggregate_gatmh_backward(c, layer - 1);
}

int dory_apply_vertex(dory_ctx *c, uint32_t layer, int dir) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (!c->prealloc) return fail(c, DORY_ERR_ARG, "apply_vertex: preallocate first");
    if (layer >= c->L) return fail(c, DORY_ERR_ARG, "apply_vertex: layer %u out of range", layer);
    const uint32_t N = c->N, Fin = c->dims[layer], Fout = c->dims[layer + 1];
    Tensor &W = c->weights[layer]["w"];
    Tensor &dW = c->wgrads[layer]["w"];
    int rc;
    if (c->gnn == DORY_GCN) {
        NEED(ah, layer, "ah");
        NEED(z, layer, "z");
        NEED(g, layer, "g");
        if (dir == DORY_FORWARD) {
            if (layer != c->L - 1) {  // vtxNNForwardGCN hidden (CPU_comm.cpp:98-107)
                NEED(h, layer, "h");
                if (tf_layer(c, layer)) {   // z_l came out of dory_aggregate already
                    GemmSend sd{};
                    int send_dir = 0;
                    bool send = false, fused = false;
                    if ((rc = rowwise_send_target(c, h, Fout, &sd, &send_dir, &send))) return rc;
                    Timed t(c, "loss", c->compute);
                    if (send) HIPCK(c, launch_tanh_forward_send(N, Fout, z->d, z->ld, h->d, h->ld, sd, c->compute, &fused));
                    else HIPCK(c, launch_tanh_forward(N, Fout, z->d, z->ld, h->d, h->ld, c->compute));
                    rowwise_sent(c, h, send_dir, sd, fused);
                } else if ((rc = gemm(c, 0, 0, N, Fout, Fin, *ah, W, *z, h))) {
                    return rc;
                }
                if (tf_layer(c, layer + 1)) {   // the next layer gathers (h_l W_{l+1}): transform before the exchange
                    NEED(xwn, layer + 1, "xw");
                    return gemm(c, 0, 0, N, c->dims[layer + 2], Fout, *h, c->weights[layer + 1]["w"], *xwn);
                }
                return DORY_OK;
            }
            // last layer (CPU_comm.cpp:108-133)
            NEED(lab, layer, "lab");
            const bool tfl = tf_layer(c, layer);   // then z_l came out of dory_aggregate, and dW_l / the handed-down gradient follow there
            if (!tfl && (rc = gemm(c, 0, 0, N, Fout, Fin, *ah, W, *z))) return rc;
            const uint32_t stt = (uint32_t)(N * 0.66);            // TRAIN_PORTION
            const uint32_t vend = stt + (uint32_t)(N * 0.1);      // VAL_PORTION
            c->val_rows = vend - stt;
            const float denom = (float)(c->globalV * 0.66);
            if ((rc = ensure_scratch(c, softmax_xent_scratch_bytes(Fout, vend - stt)))) return rc;
            {
                GemmSend sd{};
                int send_dir = 0;
                bool send = false, fused = false;
                if ((rc = rowwise_send_target(c, g, Fout, &sd, &send_dir, &send))) return rc;
                Timed t(c, "loss", c->compute);
                // maskout copies (N - stt) floats starting at dense offset stt*cols (CPU_comm.cpp:464-471)
                if (send)
                    HIPCK(c, launch_softmax_xent_send(N, Fout, z->d, z->ld, lab->d, lab->ld, g->d, g->ld, denom, stt, vend, (uint64_t)stt * Fout,
                                                      (uint64_t)(N - stt), c->d_stat, c->scratch, sd, c->compute, &fused));
                else
                    HIPCK(c, launch_softmax_xent(N, Fout, z->d, z->ld, lab->d, lab->ld, g->d, g->ld, denom, stt,
                                                 vend, (uint64_t)stt * Fout, (uint64_t)(N - stt), c->d_stat,
                                                 c->scratch, c->compute));
                rowwise_sent(c, g, send_dir, sd, fused);
            }
            if (tfl) return DORY_OK;
            if (layer > 0) {  // interGrad = d_output * W^T -> "grad"
                NEED(grad, layer, "grad");
                if ((rc = gemm(c, 0, 1, N, Fin, Fout, *g, W, *grad))) return rc;
            }
            return gemm(c, 1, 0, Fin, Fout, N, *ah, *g, dW);  // ah^T * d_output
        }
        // vtxNNBackwardGCN (CPU_comm.cpp:137-159)
        NEED(aTg, layer, "aTg");
        {
            GemmSend sd{};
            int send_dir = 0;
            bool send = false, fused = false;
            if ((rc = rowwise_send_target(c, g, Fout, &sd, &send_dir, &send))) return rc;
            Timed t(c, "loss", c->compute);
            if (send) HIPCK(c, launch_tanh_backward_send(N, Fout, aTg->d, aTg->ld, z->d, z->ld, g->d, g->ld, sd, c->compute, &fused));
            else HIPCK(c, launch_tanh_backward(N, Fout, aTg->d, aTg->ld, z->d, z->ld, g->d, g->ld, c->compute));
            rowwise_sent(c, g, send_dir, sd, fused);
        }
        if (tf_layer(c, layer)) return DORY_OK;   // dW_l (and the gradient for layer l-1) follow in dory_aggregate(l, backward)
        if ((rc = gemm(c, 1, 0, Fin, Fout, N, *ah, *g, dW))) return rc;
        if (layer != 0) {
            NEED(grad, layer, "grad");
            return gemm(c, 0, 1, N, Fin, Fout, *g, W, *grad);
        }
        return DORY_OK;
    }
    if (c->gnn == DORY_GATMH) {  // extension: z = h*W ; backward dW = h^T dz, dh = dz W^T
        NEED(hh, layer, "h");
        NEED(z, layer, "z");
        const uint32_t zw = z->cols;
        if (dir == DORY_FORWARD) return gemm(c, 0, 0, N, zw, Fin, *hh, W, *z);
        NEED(dz, layer, "dz");
        if ((rc = gemm(c, 1, 0, Fin, zw, N, *hh, *dz, dW))) return rc;
        if (layer != 0) {
            NEED(dh, layer, "dh");
            return gemm(c, 0, 1, N, Fin, zw, *dz, W, *dh);
        }
        return DORY_OK;
    }
    // GAT
    Tensor *feats = layer == 0 ? find(c, 0, "h") : find(c, layer - 1, "ah");
    if (!feats) return fail(c, DORY_ERR_ARG, "apply_vertex GAT: input missing");
    if (dir == DORY_FORWARD) {  // vtxNNForwardGAT (CPU_comm.cpp:161-169)
        NEED(z, layer, "z");
        if (layer < c->gat_nsum_valid.size()) c->gat_nsum_valid[layer] = 0;   // a new z: the kept neighbour sum of the old one no longer holds
        return gemm(c, 0, 0, N, Fout, Fin, *feats, W, *z);
    }
    // vtxNNBackwardGAT (CPU_comm.cpp:171-188)
    NEED(aTg, layer, "aTg");
    if ((rc = gemm(c, 1, 0, Fin, Fout, N, *feats, *aTg, dW))) return rc;
    if (layer != 0) {
        NEED(grad, layer - 1, "grad");
        return gemm(c, 0, 1, N, Fin, Fout, *aTg, W, *grad);
    }
    return DORY_OK;
}

int dory_apply_edge(dory_ctx *c, uint32_t layer, int dir) {
    CHECK_CTX(c);
    // dory_gatmh_row_gather_overlap: where the forward of this layer will run its interior rows beside the exchange in flight, the exchange
    // stays in flight here too -- the local scores now, the ghost sources' once it has landed (gatmh_ghost_scores_flush), the same kernels
    bool keep_flight = false;
    // dory_gatmh_row_gather_edge_split: likewise where the forward will run every row's local entries beside the exchange
    const bool ovl_ready = c->gatmh_rows_overlap && (c->adj[ADJ_IN].rows_split_built || !c->capturing);
    const bool es_ready = c->gatmh_edge_split && ((c->adj[ADJ_IN].rows_edge.built && c->adj[ADJ_IN].hub_chunk == c->gatmh_hub_chunk) || !c->capturing);
    if ((ovl_ready || es_ready) && c->halo_pending && c->gatmh_scores_pending < 0 && c->prealloc && c->gnn == DORY_GATMH && dir == DORY_FORWARD &&
        layer >= 1 && layer <= c->L && c->N && c->adj[ADJ_IN].ghosts) {
        const uint32_t l0 = layer - 1, K = c->heads[l0];
        Tensor *z = find(c, l0, "z"), *op = find(c, l0, "op"), *dpos = find(c, l0, "dpos");
        if (z && op && dpos && find(c, l0, "fg_z") && find(c, l0, "fg_el") && find(c, l0, "fg_er") && gatmh_rows_ok(K, z->cols / K, z->ld)) {
            const GatmhFwdForm form = gatmh_fwd_form(c, z, op, dpos, K, z->cols / K);
            bool split = false;
            GatmhRowList first, rest;
            bool carry = false;
            if (!form.sweep && !form.blocked && (form.rows_forced || c->numNodes > 1)) {
                int prc = ovl_ready ? gatmh_rows_lists_for(c, c->adj[ADJ_IN], &split, &first, &rest) : (int)DORY_OK;
                if (!prc && es_ready) prc = gatmh_carry_taken(c, c->adj[ADJ_IN], false, &carry);
                if (prc) return prc;
            }
            keep_flight = split || carry;
        }
    }
    if (!keep_flight) { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (!c->prealloc || c->gnn == DORY_GCN) {
        if (c->prealloc && c->gnn == DORY_GCN) return DORY_OK;  // applyEdgeGCN is a no-op (gcn_ops.cpp:364-366)
        return fail(c, DORY_ERR_ARG, "apply_edge: preallocate first");
    }
    if (layer == 0 || layer > c->L) return fail(c, DORY_ERR_ARG, "apply_edge: layer %u out of range", layer);
    if (c->gnn == DORY_GATMH) {  // extension: attention scores per vertex and head; backward lives in aggregate
        if (dir != DORY_FORWARD) return DORY_OK;
        const uint32_t l0 = layer - 1, K = c->heads[l0];
        NEED(z, l0, "z"); NEED(el, l0, "el"); NEED(er, l0, "er");
        Timed t(c, "edge", c->compute);
        HIPCK(c, launch_gatmh_scores(c->N, K, z->cols / K, z->d, z->ld, c->weights[l0]["a_l"].d, c->weights[l0]["a_r"].d,
                                     el->d, er->d, el->ld, c->compute));
        if (c->adj[ADJ_IN].ghosts) {   // scores of the ghost sources from their exchanged z rows (el is all the in-edge side needs)
            if (keep_flight) { c->gatmh_scores_pending = (int)l0; return DORY_OK; }
            return gatmh_ghost_scores(c, l0);
        }
        return DORY_OK;
    }
    const uint32_t fl = layer - 1;  // "layer--; // YIFAN: fix this" (CPU_comm.cpp:33)
    const uint32_t F = c->dims[fl + 1];
    Tensor &a = c->weights[fl]["a_i"];
    NEED(z, fl, "z");
    NEED(az, fl, "az");
    if (dir == DORY_FORWARD) {  // edgNNForwardGAT (CPU_comm.cpp:190-203)
        NEED(arow, fl, "arow");
        NEED(azrow, fl, "azrow");
        Timed t(c, "edge", c->compute);
        const bool lazy = c->opt[OPT_GAT_LAZY_EDGE_TENSORS] != 0;
        HIPCK(c, launch_edge_forward_gat(c->N, F, c->adj[ADJ_IN].ptr, z->d, z->ld, a.d, lazy ? nullptr : az->d, lazy ? nullptr : c->adj[ADJ_IN].val, arow->d,
                                         c->compute, azrow->d));
        for (auto &f : c->gat_arow_valid) f = 0;   // "A" now holds this layer's scores only
        c->gat_arow_valid[fl] = 1;
        c->gat_azrow_valid[fl] = 1;
        c->gat_az_stale[fl] = lazy ? 1 : 0;        // (lazy: the per-edge copies follow when somebody reads them, gat_materialize)
        c->gat_A_stale_layer = lazy ? (int)fl : -1;
        return DORY_OK;
    }
    // edgNNBackwardGAT (CPU_comm.cpp:205-242)
    NEED(grad, fl, "grad");
    NEED(dA, fl, "dA");
    NEED(cw, 0, "cw");
    NEED(drow, fl, "drow");
    Tensor &da = c->wgrads[fl]["a_i"];
    int rc = ensure_scratch(c, (size_t)(1024 * (size_t)F + F + c->N + 64) * sizeof(float));
    if (rc) return rc;
    float *r = c->scratch;            // F
    float *y = c->scratch + ((F + 63) & ~63u);   // N
    float *partial = y + ((c->N + 63) & ~63u);
    const size_t pbytes = c->scratch_bytes - (size_t)(partial - c->scratch) * sizeof(float);
    Timed t(c, "edge", c->compute);
    {
        Tensor *azrow = find(c, fl, "azrow");
        const bool have_row = azrow && c->gat_azrow_valid[fl];
        const bool lazy = c->opt[OPT_GAT_LAZY_EDGE_TENSORS] != 0 && have_row;
        if (!have_row) { int mrc = gat_materialize(c, fl, 1); if (mrc) return mrc; }   // (az comes from the caller, or is current already)
        HIPCK(c, launch_edge_backward_gat(c->N, F, c->adj[ADJ_IN].ptr, grad->d, grad->ld, az->d, a.d, lazy ? nullptr : dA->d, cw->d, drow->d, c->compute,
                                          have_row ? azrow->d : nullptr));
        c->gat_dA_stale[fl] = lazy ? 1 : 0;
    }
    c->gat_drow_valid[fl] = 1;
    // r = grad^T cw ; da = z^T (z r)   [= (z^T z) r^T, CPU_comm.cpp:232-236, without the F x F matrix]
    HIPCK(c, launch_colsum_w(c->N, F, grad->d, grad->ld, cw->d, partial, pbytes, r, c->compute));
    HIPCK(c, launch_rowdot(c->N, F, z->d, z->ld, r, y, c->compute));
    HIPCK(c, launch_colsum_w(c->N, F, z->d, z->ld, y, partial, pbytes, da.d, c->compute));
    return DORY_OK;
}

int dory_predict_gat(dory_ctx *c, uint32_t layer) {
    CHECK_CTX(c);
    { int wrc = wait_halo(c); if (wrc) return wrc; }
    if (!c->prealloc || c->gnn == DORY_GCN || layer == 0 || layer > c->L)
        return fail(c, DORY_ERR_ARG, "predict_gat: bad state or layer");
    const uint32_t fl = layer - 1;
    if (c->gnn == DORY_GATMH) {
        NEED(lg, fl, "logits"); NEED(lab, fl, "lab"); NEED(gr, fl, "grad");
        Timed t(c, "loss", c->compute);
        HIPCK(c, launch_softmax_sub(c->N, lg->cols, lg->d, lg->ld, lab->d, lab->ld, gr->d, gr->ld, c->compute));
        return DORY_OK;
    }
    // Engine::predictGAT (gat_ops.cpp:246-265).  The reference reads the edge tensor
    // "az" where it means the aggregated "ah" (SURVEY.md 0-6); we use "ah".
    NEED(ah, fl, "ah");
    NEED(lab, fl, "lab");
    NEED(grad, fl, "grad");
    GemmSend sd{};
    int send_dir = 0;
    bool send = false, fused = false;
    { int rc = rowwise_send_target(c, grad, c->dims[layer], &sd, &send_dir, &send); if (rc) return rc; }
    Timed t(c, "loss", c->compute);
    if (send) HIPCK(c, launch_softmax_sub_send(c->N, c->dims[layer], ah->d, ah->ld, lab->d, lab->ld, grad->d, grad->ld, sd, c->compute, &fused));
    else HIPCK(c, launch_softmax_sub(c->N, c->dims[layer], ah->d, ah->ld, lab->d, lab->ld, grad->d, grad->ld, c->compute));
    rowwise_sent(c, grad, send_dir, sd, fused);
    return DORY_OK;
}

int dory_train_stat(dory_ctx *c, float *acc_sum, float *loss_sum, uint32_t *val_rows) {
    CHECK_CTX(c);
    float h[2] = {0, 0};
    HIPCK(c, hipMemcpyAsync(h, c->d_stat, sizeof(h), hipMemcpyDeviceToHost, c->compute));
    HIPCK(c, hipStreamSynchronize(c->compute));
    if (acc_sum) *acc_sum = h[0];
    if (loss_sum) *loss_sum = h[1];
    if (val_rows) *val_rows = c->val_rows;
    return DORY_OK;
}

}  // extern "C"
