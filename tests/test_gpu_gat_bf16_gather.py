"""dory_gat_bf16_gather (include/dorylus_hip.h): the GAT prototype's aggregations read their rows rounded to bf16 (round to
nearest even) and sum in fp32.  mode 1 = the aggregations that gather z / fg_z, 2 = the backward's A^T grad too; wide = K1s
gathers rows of 128 floats or more eight features per lane.

  * exactness: ah and aTg in modes 1 / 2, narrow and wide, gat_reuse_nsum 0 and 1, are bit for bit what the same context gives
    with mode 0 on the tensors uploaded rounded -- K1s (one and two launches, split hub rows, narrow and wide) and K1 (long
    rows), the path read off the feature's counters and spmm_launches_*; random normals with the finite special values (ties,
    +-0, the next binade, fp32 subnormals);
  * the error bound on unrounded inputs against float64 (tests/gat_stage_ref.py): the fp32 bound of the module plus
    2^-8 sum |w_e| |row_e| (+ 2^-8 |z_v| for the self row) -- 2^-8 is bf16's unit roundoff, the magnitudes are the reference's;
  * schedules: two ranks with and without overlap, an epoch recorded after one eager epoch, a caller who overwrites z between
    forward and backward, a mode switched between forward and backward;
  * refusals and the default."""
import numpy as np
import pytest

import gat_stage_ref as gr
from gat_stage_ref import golden, graph
from test_gpu_bf16_gather import _golden, _graph, _inputs, bf16

pytestmark = pytest.mark.gpu

FWD, BWD = 0, 1
LAUNCH_KEYS = ("spmm_launches_k1s", "spmm_launches_k1b", "spmm_launches_k1")
NAMES = ("z", "fg_z", "grad", "bg_d")


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _make(da, g, dims, options, r=0, P=1):
    from helpers import make_ctx
    return make_ctx(da, g, dims, g["globalVtxCnt"], gnn=da.GAT, node_id=r, num_nodes=P, options=options)


def _up(ctx, layer, name, a):
    if np.size(a):
        ctx.upload(layer, name, a)


def _counts(ctx):
    """(aggregations per kernel family: K1s, K1b, K1; the feature's counters)"""
    return np.array([ctx.get_option(k) for k in LAUNCH_KEYS]), ctx.gat_bf16_gather_stats()


def _delta(c0, c1):
    return (c1[0] - c0[0]).tolist(), {k: c1[1][k] - c0[1][k] for k in c1[1]}


def _primed(da, g, F, r, P, options):
    """a one-layer context whose edge stage has run forward and backward once on modest inputs: arow / drow are in force (at
    most 1 in magnitude: a_i is scaled by 1 / F), and uploads of z do not clear them"""
    ctx = _make(da, g, [8, F], options, r, P)
    inp = gr.stage_inputs(g, F, "random")
    for nm in NAMES:
        _up(ctx, 0, nm, inp[nm])
    ctx.weight_set(0, "a_i", (inp["a"] / np.float32(F)).astype(np.float32))
    ctx.apply_edge(1, FWD)
    ctx.apply_edge(1, BWD)
    return ctx


def _special(g, F, seed):
    rng = np.random.default_rng([seed, F, int(g["localVtxCnt"])])
    rows = {"z": g["localVtxCnt"], "fg_z": g["srcGhostCnt"], "grad": g["localVtxCnt"], "bg_d": g["dstGhostCnt"]}
    return {nm: _inputs(rng, int(rows[nm]), F, finite=True) for nm in NAMES}


def _run(ctx, T, round_z, round_g):
    for nm in NAMES:
        rnd = round_z if nm in ("z", "fg_z") else round_g
        _up(ctx, 0, nm, bf16(T[nm]) if rnd else T[nm])
    ctx.aggregate(1, FWD)
    ah = ctx.download(0, "ah")
    ctx.aggregate(1, BWD)
    return ah, ctx.download(0, "aTg")


def _exact(da, label, g, F, r=0, P=1, variant=2, nb=8):
    """the issue's sequence in one context; returns the (k1s, k1s_wide, k1) bf16 aggregations seen over all runs"""
    ctx = _primed(da, g, F, r, P, {"spmm_blk_nb": nb, "spmm_variant": variant})
    T = _special(g, F, 1)
    ld = (F + 31) // 32 * 32
    seen = np.zeros(3, np.int64)
    for reuse in (0, 1):
        ctx.set_option("gat_reuse_nsum", reuse)
        for mode in (1, 2):
            what = (label, "reuse", reuse, "mode", mode)
            ctx.gat_bf16_gather(0, 0)
            c0 = _counts(ctx)
            ref = _run(ctx, T, True, mode == 2)
            dl, ds = _delta(c0, _counts(ctx))
            assert not any(ds.values()), what + (ds,)                 # mode 0: nothing counted
            n_agg = sum(dl)
            if dl[1]:      # fp32 took K1b (variant 2 without a sweep layout): bf16 takes K1 -- compare against K1
                ctx.set_option("spmm_variant", 0)
                ref = _run(ctx, T, True, mode == 2)
                ctx.set_option("spmm_variant", variant)
            assert np.count_nonzero(ref[0][:, 1 % F]) > 0.5 * ref[0].shape[0], what     # (the subnormal column survives the rounding)
            got = {}
            for wide in (0, 1):
                ctx.gat_bf16_gather(mode, wide)
                c0 = _counts(ctx)
                got[wide] = _run(ctx, T, False, False)
                dl, ds = _delta(c0, _counts(ctx))
                assert ds["fp32_fallbacks"] == 0 and dl[1] == 0, what + (wide, dl, ds)
                # every aggregation of the pair ran on bf16 rows, but (mode 1) the A^T grad gather
                assert ds["k1s"] + ds["k1"] == sum(dl) - (1 if mode == 1 else 0), what + (wide, dl, ds)
                assert ds["k1s"] <= dl[0] and ds["k1"] <= dl[2], what + (wide, dl, ds)
                if variant == 0:
                    assert dl[0] == 0 and ds["k1s"] == 0 and ds["k1"] > 0, what + (wide, dl, ds)       # spmm_variant = 0 runs K1
                elif not dl[2]:
                    assert sum(dl) == n_agg, what + (wide, dl, n_agg)                                   # the fp32 path's aggregations
                # the wide form: every K1s aggregation on bf16 rows of 128 floats or more, none below
                assert ds["k1s_wide"] == (ds["k1s"] if wide and ld >= 128 else 0), what + (wide, ld, ds)
                assert _bits(got[wide][0], ref[0]), what + (wide, "ah")
                assert _bits(got[wide][1], ref[1]), what + (wide, "aTg")
                seen += [ds["k1s"], ds["k1s_wide"], ds["k1"]]
            assert _bits(got[0][0], got[1][0]) and _bits(got[0][1], got[1][1]), what + ("narrow and wide",)
    ctx.close()
    return seen


@pytest.mark.parametrize("N,F", gr.AGG_CASES + [(300, 256)], ids=lambda v: str(v))
def test_exact_k1s(da, N, F):
    seen = _exact(da, f"N{N}-F{F}", graph(N), F)
    assert seen[0] > 0 and seen[2] == 0, seen                       # K1s throughout
    assert (seen[1] > 0) == (F >= 128), seen                        # ld < 128: wide = 1 runs the narrow form


def test_exact_k1_variant_0(da):
    seen = _exact(da, "N300-F128-k1", graph(300), 128, variant=0)
    assert seen[0] == 0 and seen[2] > 0, seen


@pytest.fixture(scope="module")
def hub_graph():
    import partition_oracle as po
    V = 1000
    s, d = _graph(2, V, 20000, hub=True)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    assert np.diff(g["colPtr"].astype(np.int64)).max() > 8192 and np.diff(g["rowPtr"].astype(np.int64)).max() > 8192
    return g


@pytest.mark.parametrize("F,variant", [(128, 2), (41, 2), (128, 0)], ids=["k1s-F128", "k1s-F41", "k1-F128"])
def test_exact_hub_rows(da, hub_graph, F, variant):
    """a destination of 12 000 in-edges and a source of 10 000 out-edges: pieces of split rows + the combine kernel in K1s (with
    the row factor and the bf16 self row), the long-row kernels in K1"""
    seen = _exact(da, f"hub-F{F}-v{variant}", hub_graph, F, variant=variant)
    if variant == 0:
        assert seen[0] == 0 and seen[2] > 0, seen
    else:
        assert seen[0] > 0, seen
        assert (seen[1] > 0) == (F >= 128), seen


@pytest.mark.parametrize("name,F", gr.AGG_GOLDENS, ids=[n for n, _ in gr.AGG_GOLDENS])
def test_exact_ghost_rows(da, name, F):
    """every rank of the goldens with ghost rows: K1s in two launches (the ghost rows are rounded after the local ones), and K1
    with the interior / boundary split forced"""
    gs = golden(name)
    for r, g in enumerate(gs):
        assert g["srcGhostCnt"] > 0 and g["dstGhostCnt"] > 0
        seen = _exact(da, f"{name}-r{r}", g, F, r, len(gs))
        assert seen[0] > 0 and seen[1] == 0 and seen[2] == 0, seen
    g = gs[0]
    ctx = _primed(da, g, F, 0, len(gs), {"spmm_variant": 0, "spmm_blk_force_split": 1})
    T = _special(g, F, 2)
    for mode in (1, 2):
        ctx.gat_bf16_gather(0, 0)
        ref = _run(ctx, T, True, mode == 2)
        ctx.gat_bf16_gather(mode, 0)
        got = _run(ctx, T, False, False)
        assert _bits(got[0], ref[0]) and _bits(got[1], ref[1]), (name, "k1 split", mode)
    assert ctx.gat_bf16_gather_stats()["k1"] > 0
    ctx.close()


# ---- the error bound on unrounded inputs ---------------------------------------------------------------------------------------
WAYS = {"k1": dict(spmm_blk_nb=0, gat_reuse_nsum=0), "unit": dict(spmm_blk_nb=8, gat_reuse_nsum=0), "nsum": dict(spmm_blk_nb=8, gat_reuse_nsum=1)}
U_BF16 = 2.0 ** -8


def _agg_partitions():
    out = [(f"N{N}-F{F}", ("graph", N), F, 0, 1) for N, F in gr.AGG_CASES]
    for name, F in gr.AGG_GOLDENS:
        out += [(f"{name}-r{r}-F{F}", ("golden", name), F, r, None) for r in range(len(golden(name)))]
    return out


AGG_PARTS = _agg_partitions()


def _magnitudes(N, ptr, idx, w, local, ghost):
    """per element: sum over the entries e of a row of |w_e| |row_e| (float64)"""
    rows = np.abs(gr._stack(local, ghost))[np.asarray(idx, np.int64)]
    return gr._gather_sum(N, gr.edge_owner(ptr), np.abs(np.asarray(w, np.float64).reshape(-1)), rows)[0]


@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("case", range(len(AGG_PARTS)), ids=[p[0] for p in AGG_PARTS])
def test_error_bound_on_unrounded_inputs(da, case, way):
    label, (kind, key), F, r, P = AGG_PARTS[case]
    gs = [graph(key)] if kind == "graph" else golden(key)
    g, P = gs[r], len(gs)
    N = g["localVtxCnt"]
    for wide in (0, 1):
        what = (label, way, "wide", wide)
        inp = gr.stage_inputs(g, F, "random")
        ctx = _make(da, g, [8, F], WAYS[way], r, P)
        ctx.gat_bf16_gather(2, wide)
        for nm in NAMES:
            _up(ctx, 0, nm, inp[nm])
        ctx.weight_set(0, "a_i", inp["a"])
        ctx.apply_edge(1, FWD)
        c0 = _counts(ctx)
        ctx.aggregate(1, FWD)
        A = ctx.download(0, "A").ravel()
        ref, b = gr.aggregate_fwd(g, A, inp["z"], inp["fg_z"])
        M = _magnitudes(N, g["colPtr"], g["rowIdx"], A, inp["z"], inp["fg_z"])
        bound = b + U_BF16 * (M + np.abs(np.asarray(inp["z"], np.float64)))
        got = ctx.download(0, "ah")
        q = gr.err_over_bound(got, ref, bound)
        print("ratio", what, "ah", f"{q:.4g}", "of which fp32 bound alone", f"{gr.err_over_bound(got, ref, b):.4g}")
        assert np.isfinite(got).all() and q <= 1.0, what + ("ah", q)
        ctx.apply_edge(1, BWD)
        ctx.aggregate(1, BWD)
        dl, ds = _delta(c0, _counts(ctx))
        assert ds["k1s"] == dl[0] and ds["k1"] == dl[2] and dl[1] == 0 and ds["fp32_fallbacks"] == 0, what + (dl, ds)
        assert (dl[0] == 0) == (way == "k1"), what + (dl,)
        dA = ctx.download(0, "dA").ravel()
        ref, b = gr.aggregate_bwd(g, inp["grad"], inp["bg_d"], dA, inp["z"], inp["fg_z"])
        M = (_magnitudes(N, g["rowPtr"], g["colIdx"], g["csrVal"], inp["grad"], inp["bg_d"]) +
             _magnitudes(N, g["colPtr"], g["rowIdx"], dA, inp["z"], inp["fg_z"]))
        got = ctx.download(0, "aTg")
        q = gr.err_over_bound(got, ref, b + U_BF16 * M)
        print("ratio", what, "aTg", f"{q:.4g}", "of which fp32 bound alone", f"{gr.err_over_bound(got, ref, b):.4g}")
        assert np.isfinite(got).all() and q <= 1.0, what + ("aTg", q)
        ctx.close()


# ---- schedules -------------------------------------------------------------------------------------------------------------------
def _epoch_inputs(V, dims, seed):
    rng = np.random.default_rng(seed)
    L = len(dims) - 1
    H0 = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]
    As = [(rng.standard_normal((dims[i + 1], 1)) / 2).astype(np.float32) for i in range(L)]
    return H0, labels, Ws, As


def test_two_ranks_overlap_on_and_off_give_the_same_weights(da):
    """parts_toy60_p2 as two contexts over the in-process device transport, three engine epochs with mode 2: the ghost rows are
    rounded only after their exchange has landed, so overlapping the local-source launches with the exchange changes no bit"""
    from local_ranks import run_local
    dims, epochs = [20, 16, 6], 3
    runs, stats = [], []
    for overlap in (1, 0):
        pobjs, parts = _golden(da, "parts_toy60_p2")
        H0, labels, Ws, As = _epoch_inputs(len(parts), dims, 5)
        seen = []

        def pre(ctx):
            ctx.gat_bf16_gather(2, 0)
            close = ctx.close

            def close_and_note():        # (run_local closes its contexts: the counters are read just before)
                seen.append(ctx.gat_bf16_gather_stats())
                close()
            ctx.close = close_and_note

        def setup(ctx, r, g):
            if g["localVtxCnt"]:
                ctx.upload(0, "h", H0[g["localToGlobal"]])
            ctx.labels_upload(labels[g["localToGlobal"]])
            for l in range(len(Ws)):
                ctx.weight_set(l, "w", Ws[l])
                ctx.weight_set(l, "a_i", As[l])
        dl = [(l, nm) for l in range(len(Ws)) for nm in ("ah", "aTg")]
        runs.append(run_local(da, pobjs, parts, dims, da.GAT, epochs, setup, {"spmm_blk_nb": 8, "halo_overlap": overlap}, downloads=dl, pre=pre))
        stats.append(seen)
    a, b = runs
    assert len(a["weights"]) == 2
    for st in stats:
        assert len(st) == 2 and all(s["k1s"] + s["k1"] > 0 and s["fp32_fallbacks"] == 0 for s in st), stats
    assert stats[0] == stats[1], stats
    for r in range(2):
        for k in a["tensors"][r]:
            assert _bits(a["tensors"][r][k], b["tensors"][r][k]), (r, k)
        for l in range(len(dims) - 1):
            for nm in ("w", "a_i"):
                assert _bits(a["weights"][r][l][nm], b["weights"][r][l][nm]), (r, l, nm)
                assert _bits(a["wgrads"][r][l][nm], b["wgrads"][r][l][nm]), (r, l, nm)


def test_recorded_epoch_replays_the_eager_bits_and_a_mode_change_drops_it(da):
    g, dims = graph(1100), [8, 128, 6]
    V = g["localVtxCnt"]
    H0, labels, Ws, As = _epoch_inputs(V, dims, 7)
    states = []
    for use_graph in (0, 1):
        ctx = _make(da, g, dims, {"spmm_blk_nb": 8})
        ctx.upload(0, "h", H0)
        ctx.labels_upload(labels)
        for l in range(2):
            ctx.weight_set(l, "w", Ws[l])
            ctx.weight_set(l, "a_i", As[l])
        ctx.adam_config(0.01)
        ctx.gat_bf16_gather(2, 1)
        ctx.set_option("epoch_graph", use_graph)
        eng = da.NativeEngine(ctx)
        eng.run(1)                       # eager: sizes what is sized lazily
        s0 = ctx.gat_bf16_gather_stats()
        eng.run(3)                       # epoch_graph = 1: recorded once, replayed
        s1 = ctx.gat_bf16_gather_stats()
        assert ctx.get_option("epoch_graph_recorded") == use_graph
        assert s0["k1s"] > 0 and s0["k1s_wide"] > 0 and s1["fp32_fallbacks"] == 0, (s0, s1)
        st = {}
        for l in range(2):
            for nm in ("w", "a_i"):
                st[(nm, l)] = ctx.weight_get(l, nm)
                st[("d" + nm, l)] = ctx.weight_grad_get(l, nm)
            for nm in ("z", "ah", "aTg"):
                st[(nm, l)] = ctx.download(l, nm)
        states.append(st)
        if use_graph:
            ctx.gat_bf16_gather(2, 1)    # the same setting: the recording stays
            assert ctx.get_option("epoch_graph_recorded") == 1
            ctx.gat_bf16_gather(1, 0)    # another mode: its kernels are not the recorded ones
            assert ctx.get_option("epoch_graph_recorded") == 0
            eng.run(2)                   # an eager epoch, then a new recording
            assert ctx.get_option("epoch_graph_recorded") == 1
        eng.close()
        ctx.close()
    for k in states[0]:
        assert _bits(states[0][k], states[1][k]), k


def _fwd_bwd(ctx, z_fwd, z_bwd, T, mode_fwd, mode_bwd):
    """forward on z_fwd under mode_fwd, then (z uploaded again if z_bwd is given) backward under mode_bwd"""
    ctx.gat_bf16_gather(mode_fwd, 0)
    for nm in ("fg_z", "grad", "bg_d"):
        _up(ctx, 0, nm, T[nm])
    ctx.upload(0, "z", z_fwd)
    ctx.aggregate(1, FWD)
    if z_bwd is not None:
        ctx.upload(0, "z", z_bwd)
    ctx.gat_bf16_gather(mode_bwd, 0)
    c0 = _counts(ctx)
    ctx.aggregate(1, BWD)
    return ctx.download(0, "aTg"), _delta(c0, _counts(ctx))


def test_overwritten_z_and_switched_mode_do_not_reuse_a_stale_nsum(da):
    g, F = graph(300), 128
    ctx = _primed(da, g, F, 0, 1, {"spmm_blk_nb": 8})
    T, T2 = _special(g, F, 3), _special(g, F, 4)
    R = dict(T, fg_z=bf16(T["fg_z"]))           # (no ghost rows here; kept for the shape of the call)
    # sanity: untouched z, mode 1 both ways -> the kept sum is reused (one aggregation in the backward)
    ctx.set_option("gat_reuse_nsum", 1)
    _, (dl, ds) = _fwd_bwd(ctx, T["z"], None, T, 1, 1)
    assert sum(dl) == 1 and ds["k1s"] == 0, (dl, ds)
    # a caller who overwrites z between forward and backward: the general path, on bf16 z
    got, (dl, ds) = _fwd_bwd(ctx, T["z"], T2["z"], T, 1, 1)
    assert dl == [2, 0, 0] and ds["k1s"] == 1, (dl, ds)
    ref, (dl, ds) = _fwd_bwd(ctx, bf16(T["z"]), bf16(T2["z"]), R, 0, 0)
    assert dl == [2, 0, 0] and not any(ds.values()), (dl, ds)
    assert _bits(got, ref)
    # the mode switched on between forward and backward: the fp32 neighbour sum is not what mode 1 asks for
    got, (dl, ds) = _fwd_bwd(ctx, T["z"], None, T, 0, 1)
    assert dl == [2, 0, 0] and ds["k1s"] == 1, (dl, ds)
    ctx.set_option("gat_reuse_nsum", 0)         # the counterpart: the general path in fp32 on rounded z
    ref, _ = _fwd_bwd(ctx, bf16(T["z"]), None, R, 0, 0)
    assert _bits(got, ref)
    # ... and switched off: the sum of rounded rows is not what mode 0 asks for
    ctx.set_option("gat_reuse_nsum", 1)
    got, (dl, ds) = _fwd_bwd(ctx, T["z"], None, T, 1, 0)
    assert dl == [2, 0, 0] and not any(ds.values()), (dl, ds)
    ctx.set_option("gat_reuse_nsum", 0)
    ref, _ = _fwd_bwd(ctx, T["z"], None, T, 0, 0)
    assert _bits(got, ref)
    assert not _bits(got, _fwd_bwd(ctx, bf16(T["z"]), None, R, 0, 0)[0])      # (the rounding is visible in these inputs)
    ctx.close()


# ---- refusals, default -------------------------------------------------------------------------------------------------------
def test_refusals(da):
    for gnn, own in ((da.GCN, "gcn_bf16_gather"), (da.GATMH, "gatmh_bf16_gather")):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        with pytest.raises(da.DoryError, match="DORY_GAT.*only"):
            ctx.gat_bf16_gather(1)
        with pytest.raises(da.DoryError, match=own):
            ctx.gat_bf16_gather(2, 1)
        assert not any(ctx.gat_bf16_gather_stats().values())
        ctx.close()
        ctx = da.Context(0)               # set on a fresh context, then configured as another model: refused there
        ctx.gat_bf16_gather(1)
        with pytest.raises(da.DoryError, match="dory_gat_bf16_gather"):
            ctx.configure(gnn, [16, 8, 3], 100)
        ctx.gat_bf16_gather(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        ctx.close()
    g, F = graph(300), 128
    ctx = _primed(da, g, F, 0, 1, {"spmm_blk_nb": 8})
    for mode, wide, cause in ((3, 0, "mode 3"), (-1, 0, "mode -1"), (1, 2, "wide 2"), (0, 1, "wide = 1 needs mode")):
        with pytest.raises(da.DoryError, match=cause):
            ctx.gat_bf16_gather(mode, wide)
    ctx.aggregate(1, FWD)
    assert not any(ctx.gat_bf16_gather_stats().values())          # none of the refused calls switched anything on
    ctx.set_option("spmm_variant", 1)
    ctx.gat_bf16_gather(1, 0)
    for d in (FWD, BWD):
        c0 = _counts(ctx)
        mark = ctx.download(0, "ah" if d == FWD else "aTg")
        with pytest.raises(da.DoryError, match="spmm_variant = 1"):
            ctx.aggregate(1, d)
        dl, ds = _delta(c0, _counts(ctx))
        assert not any(dl) and not any(ds.values()), (dl, ds)       # nothing launched
        assert _bits(ctx.download(0, "ah" if d == FWD else "aTg"), mark)
    ctx.gat_bf16_gather(0, 0)
    ctx.aggregate(1, FWD)                                          # (fp32 K1b as before)
    ctx.close()


def test_default_is_off_and_setting_it_off_changes_nothing(da):
    g, dims = graph(300), [8, 128, 6]
    H0, labels, Ws, As = _epoch_inputs(g["localVtxCnt"], dims, 9)
    states = []
    for touch in (0, 1):
        ctx = _make(da, g, dims, {"spmm_blk_nb": 8})
        if touch:
            ctx.gat_bf16_gather(0, 0)
        ctx.upload(0, "h", H0)
        ctx.labels_upload(labels)
        for l in range(2):
            ctx.weight_set(l, "w", Ws[l])
            ctx.weight_set(l, "a_i", As[l])
        ctx.adam_config(0.01)
        eng = da.NativeEngine(ctx)
        eng.run(2)
        assert not any(ctx.gat_bf16_gather_stats().values())
        st = {(nm, l): ctx.download(l, nm) for l in range(2) for nm in ("z", "ah", "aTg", "nsum")}
        st.update({("w" + nm, l): ctx.weight_get(l, nm) for l in range(2) for nm in ("w", "a_i")})
        states.append(st)
        eng.close()
        ctx.close()
    for k in states[0]:
        assert _bits(states[0][k], states[1][k]), k
