"""dory_k1_bf16_wide (include/dorylus_hip.h): K1's aggregations on bf16 rows gather 16 bytes a lane (spmm_rows_bf16x8_kernel), and no
bit of any result changes against the switch being off.  Every comparison is bit for bit; there is no tolerance in this file.

  * exact values (aggregate_ref: integer features, signed powers of two as weights): every aggregation is the float64 reference,
    narrow and wide, in every direction, over one width per instantiation and the edges of the rule (k1_bf16_wide_ref.WIDTHS), on
    a 203-row graph with ghost rows, multi-edges, self loops and a degree planted at every boundary of the kernel's loops; with
    spmm_blk_force_split the same widths run the two-launch edge split (accumulate == 2) and the row split;
  * ordinary values (uniform features, GCN's own edge values): wide = narrow;
  * schedules (spmm_order, spmm_edge_split, spmm_blk_force_split) on a partition of 150 local and 90 ghost rows; long rows; the GAT
    prototype; whole epochs on two ranks over the in-process transport with ghost twins; a replayed epoch graph; the setter.
All cases run with spmm_variant = 0, so K1 runs; the counters of dory_k1_bf16_wide_stats say which form did."""
import numpy as np
import pytest

import aggregate_ref as ar
import k1_bf16_wide_ref as kr

pytestmark = pytest.mark.gpu

WIDTH_IDS = [f"F{F}" + (f"_slab{s}" if s else "") for F, s, _ in kr.WIDTHS]
ZERO = {"wide": 0, "narrow_while_on": 0}


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)      # -0 -> +0 (the sign of a zero sum depends on the order)


def _raw(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _tensors(da, direction):
    return {"fwd0": (0, da.FORWARD, (0, "x"), (0, "fg"), (0, "ah")),
            "fwd1": (1, da.FORWARD, (0, "h"), (1, "fg"), (1, "ah")),
            "bwd": (1, da.BACKWARD, (1, "grad"), (0, "bg"), (0, "aTg"))}[direction]


def _gcn_ctx(da, g, F, options=None):
    from helpers import make_ctx
    ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), options=dict({"spmm_variant": 0, "gcn_bf16_gather": 2}, **(options or {})))
    assert ctx.k1_bf16_wide_stats() == ZERO
    return ctx


def _upload(ctx, da, g, direction, F, exact):
    """the rows of one aggregation; returns (local rows, ghost rows)"""
    _, _, xl_name, xg_name, _ = _tensors(da, direction)
    if exact:
        x, xg = ar.features(g, direction, F, True)
    else:
        rng = np.random.default_rng([71, F, len(direction)])
        x = rng.uniform(-1, 1, (int(g["localVtxCnt"]), F)).astype(np.float32)
        xg = rng.uniform(-1, 1, (ar.side(g, direction)[3], F)).astype(np.float32)
    ctx.upload(xl_name[0], xl_name[1], x)
    if len(xg):
        ctx.upload(xg_name[0], xg_name[1], xg)
    return x, xg


def _aggregate(ctx, da, direction, on, shape):
    """one aggregation with the switch at `on` into an output poisoned with NaN: (the output, what the switch's counters and K1's
    launch counter moved by)"""
    layer, dirn, _, _, out = _tensors(da, direction)
    ctx.k1_bf16_wide(on)
    ctx.upload(out[0], out[1], np.full(shape, np.nan, np.float32))
    s0, k0 = ctx.k1_bf16_wide_stats(), ctx.get_option("spmm_launches_k1")
    ctx.aggregate(layer, dirn)
    s1 = ctx.k1_bf16_wide_stats()
    got = ctx.download(out[0], out[1])
    return got, {k: s1[k] - s0[k] for k in s1}, ctx.get_option("spmm_launches_k1") - k0


def _reference(g, direction, x, xg):
    ptr, idx, val, _ = ar.side(g, direction)
    ar.exact_ok(ptr, idx, val, g["norm"], x, xg, 1)
    ref = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1)
    ref32 = ref.astype(np.float32)
    assert (ref32.astype(np.float64) == ref).all()
    return ref32


def _off_and_on(ctx, da, direction, shape, has_form, what, ref32=None):
    """the aggregation with the switch off and on: the same bits (the reference's, where there is one), the right counter moved"""
    narrow, moved, k1 = _aggregate(ctx, da, direction, 0, shape)
    assert moved == ZERO and k1 == 1, (what, "off", moved, k1)
    wide, moved, k1 = _aggregate(ctx, da, direction, 1, shape)
    assert moved == ({"wide": 1, "narrow_while_on": 0} if has_form else {"wide": 0, "narrow_while_on": 1}) and k1 == 1, (what, "on", moved, k1)
    if ref32 is not None:
        for name, got in (("narrow", narrow), ("wide", wide)):
            bad = np.nonzero((_bits(got) != _bits(ref32)).any(axis=1))[0]
            assert bad.size == 0, (what, name, "rows that differ from the reference", bad.size, bad[:8].tolist(),
                                   "got", got[bad[0], :4].tolist(), "want", ref32[bad[0], :4].tolist())
    bad = np.nonzero((_raw(wide) != _raw(narrow)).any(axis=1))[0]
    assert bad.size == 0, (what, "rows where wide differs from narrow", bad.size, bad[:8].tolist())
    assert not np.isnan(wide).any(), (what, "a row nobody wrote")
    ctx.k1_bf16_wide(0)


# ---- every instantiation, every edge of the rule ------------------------------------------------------------------------------
@pytest.mark.parametrize("F,slab,want", kr.WIDTHS, ids=WIDTH_IDS)
def test_exact_values_equal_the_reference_narrow_and_wide(da, F, slab, want):
    g = kr.graph203("exact")
    ctx = _gcn_ctx(da, g, F, {"spmm_slab": slab})
    assert da.k1_bf16_wide_form(ar.pad_ld(F), slab) == (want[:2] if want else None)
    for direction in ar.DIRECTIONS:
        x, xg = _upload(ctx, da, g, direction, F, True)
        ref32 = _reference(g, direction, x, xg)
        for split in (0, 1):      # 1: the local-first copy in two launches (fwd1, bwd: the second goes on from the first's sums), the row split (fwd0)
            ctx.set_option("spmm_blk_force_split", split)
            _off_and_on(ctx, da, direction, ref32.shape, want is not None, (F, slab, direction, "split", split), ref32)
        ctx.set_option("spmm_blk_force_split", 0)
    ctx.close()


@pytest.mark.parametrize("F,slab,want", kr.WIDTHS, ids=WIDTH_IDS)
def test_ordinary_values_wide_equals_narrow(da, F, slab, want):
    g = kr.graph203("real")
    ctx = _gcn_ctx(da, g, F, {"spmm_slab": slab})
    for direction in ar.DIRECTIONS:
        _upload(ctx, da, g, direction, F, False)
        for split in (0, 1):
            ctx.set_option("spmm_blk_force_split", split)
            _off_and_on(ctx, da, direction, (kr.N_ROWS, F), want is not None, (F, slab, direction, "split", split))
        ctx.set_option("spmm_blk_force_split", 0)
    ctx.close()


# ---- schedules that must not change a bit -----------------------------------------------------------------------------------------
SCHEDULES = [{}, {"spmm_order": 0}, {"spmm_order": 2}, {"spmm_edge_split": 0}, {"spmm_blk_force_split": 1},
             {"spmm_blk_force_split": 1, "spmm_edge_split": 0}, {"spmm_blk_force_split": 1, "spmm_order": 2},
             {"spmm_blk_force_split": 1, "spmm_order": 0, "spmm_edge_split": 0}]
SCHEDULE_DEFAULTS = {"spmm_order": 1, "spmm_edge_split": 1, "spmm_blk_force_split": 0}


@pytest.mark.parametrize("F", [41, 300, 602])
@pytest.mark.parametrize("values", ["exact", "real"])
def test_schedules_on_a_partition_with_ghosts(da, F, values):
    """150 local and 90 ghost rows: fwd1 walks the two-launch edge split with boundary rows, bwd the side whose ghosts no edge reads
    (no second launch), fwd0 and spmm_edge_split = 0 the interior / boundary row split"""
    g = kr.partition150(values)
    ctx = _gcn_ctx(da, g, F)
    for direction in ar.DIRECTIONS:
        x, xg = _upload(ctx, da, g, direction, F, values == "exact")
        ref32 = _reference(g, direction, x, xg) if values == "exact" else None
        first = None
        for sched in SCHEDULES:
            for k, v in dict(SCHEDULE_DEFAULTS, **sched).items():
                ctx.set_option(k, v)
            _off_and_on(ctx, da, direction, (kr.P_LOCAL, F), True, (F, values, direction, sched), ref32)
            got = _aggregate(ctx, da, direction, 1, (kr.P_LOCAL, F))[0]
            if values == "exact":
                first = got if first is None else first
                assert np.array_equal(_bits(got), _bits(first)), (F, direction, sched, "the schedule changed a bit")
        ctx.k1_bf16_wide(0)
    ctx.close()


# ---- long rows ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [100, 602])
def test_long_rows_wide_launch_beside_narrow_chunk_kernels(da, F):
    """a row of LONG_ROW_CLAMP + LONG_ROW_CHUNK + 3 entries: K1's clamped launch runs wide, the chunk kernels narrow"""
    for values in ("exact", "real"):
        g = kr.graph203(values, True)
        ctx = _gcn_ctx(da, g, F)
        for direction in ar.DIRECTIONS:
            ptr = ar.side(g, direction)[0]
            assert int(np.diff(ptr.astype(np.int64)).max()) == kr.LONG_ROW
            x, xg = _upload(ctx, da, g, direction, F, values == "exact")
            ref32 = _reference(g, direction, x, xg) if values == "exact" else None
            _off_and_on(ctx, da, direction, (kr.N_ROWS, F), True, (F, values, direction, "long row"), ref32)
        ctx.close()


# ---- the GAT prototype --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [41, 100, 602])
def test_gat_prototype_k1_wide_equals_narrow(da, F):
    """a DORY_GAT context with dory_gat_bf16_gather(2, 0) and spmm_variant = 0: both aggregations of a layer run K1 on bf16 rows with
    the edge stage's per-edge values; ah and aTg are the same bits with the switch on and off"""
    from helpers import make_ctx
    g = kr.graph203("real")
    N = kr.N_ROWS
    ctx = make_ctx(da, g, [8, F], int(g["globalVtxCnt"]), gnn=da.GAT, options={"spmm_variant": 0})
    rng = np.random.default_rng([73, F])
    for nm, rows in (("z", N), ("fg_z", kr.N_SRC_GHOSTS), ("grad", N), ("bg_d", kr.N_DST_GHOSTS)):
        ctx.upload(0, nm, rng.uniform(-1, 1, (rows, F)).astype(np.float32))
    ctx.weight_set(0, "a_i", (rng.standard_normal((F, 1)) / F).astype(np.float32))
    ctx.apply_edge(1, da.FORWARD)
    ctx.apply_edge(1, da.BACKWARD)
    ctx.k1_bf16_wide(1)                       # inert while no gather mode is on
    ctx.aggregate(1, da.FORWARD)
    assert ctx.k1_bf16_wide_stats() == ZERO
    ctx.gat_bf16_gather(2, 0)
    out = {}
    for on in (0, 1):
        ctx.k1_bf16_wide(on)
        s0, g0 = ctx.k1_bf16_wide_stats(), ctx.gat_bf16_gather_stats()
        for nm in ("ah", "aTg"):
            ctx.upload(0, nm, np.full((N, F), np.nan, np.float32))
        ctx.aggregate(1, da.FORWARD)
        ah = ctx.download(0, "ah")
        ctx.aggregate(1, da.BACKWARD)
        out[on] = (ah, ctx.download(0, "aTg"))
        s1, g1 = ctx.k1_bf16_wide_stats(), ctx.gat_bf16_gather_stats()
        k1 = g1["k1"] - g0["k1"]
        assert k1 >= 2 and g1["k1s"] == g0["k1s"] and g1["fp32_fallbacks"] == g0["fp32_fallbacks"], (F, on, g0, g1)
        assert (s1["wide"] - s0["wide"], s1["narrow_while_on"] - s0["narrow_while_on"]) == ((k1, 0) if on else (0, 0)), (F, on, s0, s1, k1)
    for i, nm in enumerate(("ah", "aTg")):
        assert not np.isnan(out[1][i]).any(), (F, nm)
        assert np.array_equal(_raw(out[0][i]), _raw(out[1][i])), (F, nm)
    ctx.close()


# ---- whole epochs --------------------------------------------------------------------------------------------------------------------
EPOCH_DIMS = [100, 64, 41]                # 128-, 64- and 64-float rows: every aggregation of the epoch has a wide form
EPOCH_DL = [(l, nm) for l in range(2) for nm in ("ah", "z")] + [(0, "h"), (0, "aTg"), (1, "grad")]


def _epoch_case(da, V=3000, E=20000, P=2):
    rng = np.random.default_rng(79)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    parts = rng.integers(0, P, V).astype(np.int32)
    X = rng.uniform(-1, 1, (V, EPOCH_DIMS[0])).astype(np.float32)
    labels = rng.integers(0, EPOCH_DIMS[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((EPOCH_DIMS[i], EPOCH_DIMS[i + 1])) / np.sqrt(EPOCH_DIMS[i])).astype(np.float32) for i in range(2)]
    return src, dst, parts, X, labels, Ws


def _epochs(da, case, on, opts, epochs=3):
    from local_ranks import run_local
    src, dst, parts, X, labels, Ws = case
    pobjs = [da.Partition.build(src, dst, parts, r, 2) for r in range(2)]
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "x", X[g["localToGlobal"]])
        ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), EPOCH_DIMS[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
        ctx.halo_bf16_rows(1)
        ctx.halo_bf16_ghosts(1)
        ctx.k1_bf16_wide(on)
        close = ctx.close

        def closing():        # run_local closes its contexts: read the counters of every rank just before that
            if ctx.h:
                kept[r] = dict(ctx.k1_bf16_wide_stats(), twin_reads=ctx.halo_bf16_ghosts_stats()["conversions_skipped"],
                               k1=ctx.get_option("gcn_bf16_gathers_k1"), k1s=ctx.get_option("gcn_bf16_gathers_k1s"))
            close()
        ctx.close = closing

    out = run_local(da, pobjs, parts, EPOCH_DIMS, da.GCN, epochs, setup, dict(opts, spmm_variant=0, gcn_bf16_gather=2), downloads=EPOCH_DL)
    return out, kept


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("direct", [0, 1])
def test_two_rank_epochs_with_ghost_twins_same_bits(da, overlap, direct):
    """three engine epochs on two ranks of a 3000-vertex graph over the in-process transport, bf16 wire and ghost twins on: every
    weight, weight gradient and downloaded tensor the same with the switch on and off; K1 ran wide on both ranks and read the twins"""
    case = _epoch_case(da)
    opts = {"halo_overlap": overlap, "halo_direct_recv": direct}
    on, kon = _epochs(da, case, 1, opts)
    off, koff = _epochs(da, case, 0, opts)
    for r in range(2):
        assert set(on["tensors"][r]) == set(off["tensors"][r]) == set(EPOCH_DL)
        for k in EPOCH_DL:
            assert np.array_equal(_raw(on["tensors"][r][k]), _raw(off["tensors"][r][k])), (overlap, direct, r, k)
            assert np.isfinite(on["tensors"][r][k]).all(), (r, k)
        for l in range(2):
            assert np.array_equal(_raw(on["weights"][r][l]["w"]), _raw(off["weights"][r][l]["w"])), (overlap, direct, r, l, "W")
            assert np.array_equal(_raw(on["wgrads"][r][l]["w"]), _raw(off["wgrads"][r][l]["w"])), (overlap, direct, r, l, "dW")
        # three aggregations an epoch, all on K1, all with a form: layer 0's forward, layer 1's forward and backward (twins)
        assert kon[r]["k1"] == koff[r]["k1"] == 9 and kon[r]["k1s"] == 0, (r, kon[r], koff[r])
        assert (kon[r]["wide"], kon[r]["narrow_while_on"]) == (9, 0) and (koff[r]["wide"], koff[r]["narrow_while_on"]) == (0, 0), (r, kon[r], koff[r])
        assert kon[r]["twin_reads"] == koff[r]["twin_reads"] == 6, (r, kon[r], koff[r])      # the wide launches gathered the twins


def _one_rank(da, dims=(100, 64, 41), V=1500, E=9000):
    import partition_oracle as po
    rng = np.random.default_rng(83)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    g = po.preprocess(np.concatenate([s, d]), np.concatenate([d, s]), np.zeros(V, np.int64), 0, 1)
    ctx = da.Context(0)
    ctx.configure(da.GCN, list(dims), V)
    ctx.set_option("spmm_variant", 0)
    ctx.set_option("gcn_bf16_gather", 2)
    ctx.graph_upload(g)
    ctx.preallocate()
    ctx.fill_uniform(0, "x", 3, -1.0, 1.0, g["localToGlobal"])
    ctx.labels_upload(rng.integers(0, dims[-1], V).astype(np.uint32))
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    return ctx


def _epoch_by_hand(ctx, da):
    ctx.aggregate(0, da.FORWARD); ctx.apply_vertex(0, da.FORWARD)
    ctx.aggregate(1, da.FORWARD); ctx.apply_vertex(1, da.FORWARD); ctx.weight_update(1)
    ctx.aggregate(1, da.BACKWARD); ctx.apply_vertex(0, da.BACKWARD); ctx.weight_update(0)


def _state(ctx):
    out = {("w", l): ctx.weight_get(l, "w") for l in range(2)}
    out.update({("dw", l): ctx.weight_grad_get(l, "w") for l in range(2)})
    out.update({(nm, l): ctx.download(l, nm) for l in range(2) for nm in ("ah", "z")})
    out[("aTg", 0)] = ctx.download(0, "aTg")
    return out


def test_a_replayed_epoch_graph_equals_the_eager_epoch_and_a_change_drops_it(da):
    """two epochs with the switch on: eager + eager against eager + one replay of a recording; the recording holds the wide launches,
    setting the same value keeps it, another value drops it; the setter is refused while recording"""
    states = []
    for replay in (0, 1):
        ctx = _one_rank(da)
        ctx.k1_bf16_wide(1)
        eng = da.NativeEngine(ctx)
        eng.run(1)
        assert ctx.k1_bf16_wide_stats() == {"wide": 3, "narrow_while_on": 0}
        if replay:
            ctx.epoch_graph_begin()
            with pytest.raises(da.DoryError, match="recorded"):
                ctx.k1_bf16_wide(0)
            _epoch_by_hand(ctx, da)
            ctx.epoch_graph_end()
            assert ctx.k1_bf16_wide_stats() == {"wide": 6, "narrow_while_on": 0}      # recordings count, replays do not
            ctx.k1_bf16_wide(1)               # the same value: the recording stays
            ctx.epoch_graph_launch(1)
            ctx.sync()
            assert ctx.k1_bf16_wide_stats() == {"wide": 6, "narrow_while_on": 0}
        else:
            eng.run(1)
        states.append(_state(ctx))
        if replay:
            ctx.k1_bf16_wide(0)               # another value: its launches are not the recorded ones
            with pytest.raises(da.DoryError):
                ctx.epoch_graph_launch(1)
        eng.close()
        ctx.close()
    assert states[0].keys() == states[1].keys()
    for k in states[0]:
        assert np.array_equal(_raw(states[0][k]), _raw(states[1][k])), k


# ---- the setter -------------------------------------------------------------------------------------------------------------------------
def test_the_setter_default_refusals_inert_and_counters(da):
    g = kr.graph203("exact")
    F = 100
    ctx = _gcn_ctx(da, g, F, {"gcn_bf16_gather": 0})
    _upload(ctx, da, g, "fwd1", F, True)
    off = _aggregate(ctx, da, "fwd1", 0, (kr.N_ROWS, F))
    on = _aggregate(ctx, da, "fwd1", 1, (kr.N_ROWS, F))          # no gather mode: inert, fp32 rows, nothing counted
    assert off[1] == on[1] == ZERO and np.array_equal(_raw(off[0]), _raw(on[0]))
    for bad in (2, -1, 7):
        with pytest.raises(da.DoryError, match="neither 0 nor 1"):
            ctx.k1_bf16_wide(bad)
    ctx.set_option("gcn_bf16_gather", 1)                         # forward aggregations only
    assert _aggregate(ctx, da, "fwd1", 1, (kr.N_ROWS, F))[1] == {"wide": 1, "narrow_while_on": 0}
    _upload(ctx, da, g, "bwd", F, True)
    assert _aggregate(ctx, da, "bwd", 1, (kr.N_ROWS, F))[1] == ZERO
    ctx.k1_bf16_wide(0)
    assert ctx.k1_bf16_wide_stats() == {"wide": 1, "narrow_while_on": 0}      # setting it does not reset the counters
    ctx.close()
    # the default of a fresh context is off: an aggregation on bf16 rows counts nothing
    ctx = _gcn_ctx(da, g, F)
    _upload(ctx, da, g, "fwd1", F, True)
    layer, dirn, _, _, _ = _tensors(da, "fwd1")
    ctx.aggregate(layer, dirn)
    assert ctx.k1_bf16_wide_stats() == ZERO and ctx.get_option("gcn_bf16_gathers_k1") == 1
    ctx.close()
    # the multi-head GAT has its own switch
    ctx = da.Context(0)
    ctx.k1_bf16_wide(1)                                          # before configure: legal
    ctx.k1_bf16_wide(0)
    ctx.configure(da.GATMH, [16, 32, 4], 100)
    with pytest.raises(da.DoryError, match="dory_gatmh_row_gather_bf16_wide"):
        ctx.k1_bf16_wide(1)
    ctx.k1_bf16_wide(0)                                          # off is legal anywhere
    ctx.close()
