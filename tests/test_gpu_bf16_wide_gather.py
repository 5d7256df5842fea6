"""Option gcn_bf16_wide (include/dorylus_hip.h): K1s gathers the bf16 rows of option gcn_bf16_gather eight features per lane with
16-byte loads where the rows are 128 floats or wider (csrc/spmm.hip: spmm_sweep_bf16x8_kernel).  The contract is that no bit of any
result changes:

  * the option itself: default 0, values outside {0, 1} and non-GCN contexts refused, the counter read-only and 0 at the start;
  * exact values: each of the 69 aggregations of aggregate_ref.CASES that take the wide form (tests/bf16_wide_ref.py; proved to be 69,
    and to reach every instantiated form, by tests/test_bf16_wide_reference.py) equals the float64 reference bit for bit, over the
    schedules that must not change a bit, with gcn_bf16_gathers_k1s_wide and spmm_launches_k1s moved by exactly one each;
  * GCN's own edge values and normal features: wide equals narrow (gcn_bf16_wide = 0) bit for bit -- stronger than any bound;
  * the fall-backs (rows narrower than 128 floats, K1, a forced 6 or 8 rows per lane group) run as before: the wide counter stays;
  * three engine epochs, eager and through a recorded epoch graph, and two ranks on the in-process transport with the halo
    exchange overlapped and not: the same weights and tensors with the option on and off."""
import glob
import os

import numpy as np
import pytest

import aggregate_ref as ar
import bf16_wide_ref as bw

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDE, K1S, BF_K1S = "gcn_bf16_gathers_k1s_wide", "spmm_launches_k1s", "gcn_bf16_gathers_k1s"
COUNTERS = (WIDE, K1S, BF_K1S, "spmm_launches_k1", "spmm_launches_k1b")
# the schedules walked inside one aggregation: none changes a bit, every one runs the wide form
WALK = [{}, {"spmm_blk_force_split": 1}, {"spmm_sweep_loader": 0}, {"spmm_order": 0}, {"spmm_order": 2}, {"spmm_sweep_flags": 8},
        {"spmm_blk_force_split": 1, "spmm_sweep_loader": 0}]
WALK_DEFAULTS = {"spmm_blk_force_split": 0, "spmm_sweep_loader": 1, "spmm_order": 1, "spmm_sweep_flags": 0}


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


@pytest.fixture(scope="module", autouse=True)
def mirror_applies(da):
    """the list of wide aggregations comes from the mirror, which assumes 8 XCDs of 32 CUs: on another device the whole module is
    skipped (the only skip there is), with the reason"""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    ctx = da.Context(0)
    xcds = ctx.get_option("spmm_xcd_count")
    ctx.close()
    if not (xcds == 8 and cus // 8 == ar.CUS_PER_XCD):
        reason = f"the dispatch mirror assumes 8 XCDs of {ar.CUS_PER_XCD} CUs; this device has {xcds} XCDs and {cus} CUs"
        print("tests/test_gpu_bf16_wide_gather.py skipped:", reason)
        pytest.skip(reason)


def _tensors(da, direction):
    return {"fwd0": (0, da.FORWARD, (0, "x"), (0, "fg"), (0, "ah")),
            "fwd1": (1, da.FORWARD, (0, "h"), (1, "fg"), (1, "ah")),
            "bwd": (1, da.BACKWARD, (1, "grad"), (0, "bg"), (0, "aTg"))}[direction]


class Held:
    """one context per case and value mode, shared by the case's three directions (the case is the outermost parameter)"""

    def __init__(self):
        self.key, self.ctx, self.data = None, None, {}

    def close(self):
        if self.ctx is not None:
            self.ctx.close()
        self.key, self.ctx, self.data = None, None, {}

    def get(self, da, key, g, F, options, exact):
        from helpers import make_ctx
        if self.key != key:
            self.close()
            self.ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), options=options)
            self.key = key
            for direction in ar.DIRECTIONS:
                ptr, idx, val, _ = ar.side(g, direction)
                x, xg = ar.features(g, direction, F, exact)
                _, _, xl_name, xg_name, _ = _tensors(da, direction)
                self.ctx.upload(xl_name[0], xl_name[1], x)
                self.ctx.upload(xg_name[0], xg_name[1], xg)
                if exact:
                    ar.exact_ok(ptr, idx, val, g["norm"], x, xg, 1)
                    ref = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1)
                    ref32 = ref.astype(np.float32)
                    assert (ref32.astype(np.float64) == ref).all()
                    self.data[direction] = ref32
        return self.ctx


@pytest.fixture(scope="module")
def held():
    h = Held()
    yield h
    h.close()


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)      # -0 -> +0 (the reference has no signed zeros)


def _raw(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _set(ctx, variant, wide, setting=None, gather=2):
    ctx.set_option("spmm_variant", variant)
    ctx.set_option("gcn_bf16_gather", gather)
    ctx.set_option("gcn_bf16_wide", wide)
    for k, v in WALK_DEFAULTS.items():
        ctx.set_option(k, (setting or {}).get(k, v))


def _reset(ctx):
    _set(ctx, 2, 0, None, 0)


def _aggregate(ctx, da, direction, poison=True):
    """one aggregation into an output poisoned with NaN; (result, how far every counter moved)"""
    layer, dirn, _, _, out = _tensors(da, direction)
    if poison:
        rows, cols = ctx.info(out[0], out[1])[:2]
        ctx.upload(out[0], out[1], np.full((rows, cols), np.nan, np.float32))
    before = {k: ctx.get_option(k) for k in COUNTERS}
    ctx.aggregate(layer, dirn)
    moved = {k: ctx.get_option(k) - before[k] for k in COUNTERS}
    return ctx.download(out[0], out[1]), moved


def _ran_wide(moved):
    return moved[WIDE] == 1 and moved[K1S] == 1 and moved[BF_K1S] == 1 and moved["spmm_launches_k1"] == 0 and moved["spmm_launches_k1b"] == 0


# ---- the option ---------------------------------------------------------------------------------------------------------------------------
def test_option_contract(da):
    from helpers import make_ctx
    g = ar.graph("uniform:1025:12000")
    ctx = make_ctx(da, g, [128, 128, 3], 1025, options={"spmm_blk_nb": 8})
    assert ctx.get_option("gcn_bf16_wide") == 0 and ctx.get_option(WIDE) == 0
    for bad in (2, -1, 3, 100):
        with pytest.raises(da.DoryError):
            ctx.set_option("gcn_bf16_wide", bad)
    assert ctx.get_option("gcn_bf16_wide") == 0
    with pytest.raises(da.DoryError):
        ctx.set_option(WIDE, 5)                       # read-only
    for v in (0, 1, 2):                               # gcn_bf16_gather keeps its values
        ctx.set_option("gcn_bf16_gather", v)
    with pytest.raises(da.DoryError):
        ctx.set_option("gcn_bf16_gather", 3)
    # no effect while gcn_bf16_gather is 0: fp32 rows, same bits as with the option off, nothing counted
    x, _ = ar.features(g, "fwd0", 128, False)
    ctx.upload(0, "x", x)
    _set(ctx, 2, 0, gather=0)
    ref, moved = _aggregate(ctx, da, "fwd0")
    assert moved[K1S] == 1 and moved[BF_K1S] == 0 and moved[WIDE] == 0
    _set(ctx, 2, 1, gather=0)
    got, moved = _aggregate(ctx, da, "fwd0")
    assert moved[K1S] == 1 and moved[BF_K1S] == 0 and moved[WIDE] == 0 and np.array_equal(_raw(got), _raw(ref))
    # gcn_bf16_gather = 1: the forward aggregations only
    _set(ctx, 2, 1, gather=1)
    assert _ran_wide(_aggregate(ctx, da, "fwd0")[1]) and _ran_wide(_aggregate(ctx, da, "fwd1")[1])
    assert _aggregate(ctx, da, "bwd")[1][WIDE] == 0
    assert ctx.get_option(WIDE) == 2
    ctx.close()
    for gnn in (da.GAT, da.GATMH):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        with pytest.raises(da.DoryError):
            ctx.set_option("gcn_bf16_wide", 1)
        ctx.set_option("gcn_bf16_wide", 0)
        assert ctx.get_option("gcn_bf16_wide") == 0
        ctx.close()
    ctx = da.Context(0)                               # set on a fresh context, then configured as GAT: refused there
    ctx.set_option("gcn_bf16_wide", 1)
    with pytest.raises(da.DoryError):
        ctx.configure(da.GAT, [16, 8, 3], 100)
    ctx.set_option("gcn_bf16_wide", 0)
    ctx.configure(da.GAT, [16, 8, 3], 100)
    ctx.close()


# ---- the 69 aggregations ------------------------------------------------------------------------------------------------------------------
WIDE_AGGREGATIONS = bw.wide_aggregations()
PARAMS = [pytest.param(case, direction, id=f"{case[0]}-{direction}") for case, direction, _, _ in WIDE_AGGREGATIONS]


def test_the_list_is_the_sixty_nine():
    assert len(PARAMS) == 69 and {c[0] for c, _, _, _ in WIDE_AGGREGATIONS} == set(bw.EXPECTED)


@pytest.mark.parametrize("case,direction", PARAMS)
def test_wide_exact(da, held, case, direction):
    """bit for bit against the float64 reference on exact inputs (aggregate_ref.exact_ok), over the walk of the schedules; output
    poisoned with NaN before every aggregation; the first setting aggregated twice into the same context"""
    cid, gname, F, options = case
    g = ar.graph(gname)
    ctx = held.get(da, (cid, "exact"), g, F, options, True)
    want = _bits(held.data[direction])
    for setting in WALK:
        _set(ctx, 2, 1, setting)
        got, moved = _aggregate(ctx, da, direction)
        assert _ran_wide(moved), (cid, direction, setting, moved)
        bad = np.nonzero((_bits(got) != want).any(axis=1))[0]
        assert bad.size == 0, (cid, direction, setting, "rows that differ", bad.size, bad[:8].tolist(), "got", got[bad[0], :8].tolist(),
                               "want", held.data[direction][bad[0], :8].tolist())
        if not setting:
            got, moved = _aggregate(ctx, da, direction, poison=False)
            assert _ran_wide(moved) and np.array_equal(_bits(got), want), (cid, direction, "second aggregation")
    # the narrow form on the same context, for the record that the counter tells the two apart
    _set(ctx, 2, 0)
    got, moved = _aggregate(ctx, da, direction)
    assert moved[WIDE] == 0 and moved[K1S] == 1 and moved[BF_K1S] == 1 and np.array_equal(_bits(got), want), (cid, direction, moved)
    _reset(ctx)


@pytest.mark.parametrize("case,direction", PARAMS)
def test_wide_equals_narrow_on_real_values(da, held, case, direction):
    """GCN's own edge values and norm, normal features: the wide result is the narrow result, every bit (signed zeros included)"""
    cid, gname, F, options = case
    g = ar.graph(gname, "real")
    ctx = held.get(da, (cid, "real"), g, F, options, False)
    for setting in ({}, {"spmm_blk_force_split": 1}, {"spmm_sweep_loader": 0}):
        _set(ctx, 2, 0, setting)
        narrow, moved = _aggregate(ctx, da, direction)
        assert moved[WIDE] == 0 and moved[K1S] == 1 and moved[BF_K1S] == 1, (cid, direction, setting, moved)
        assert np.isfinite(narrow).all()
        _set(ctx, 2, 1, setting)
        wide, moved = _aggregate(ctx, da, direction)
        assert _ran_wide(moved), (cid, direction, setting, moved)
        bad = np.nonzero((_raw(wide) != _raw(narrow)).any(axis=1))[0]
        assert bad.size == 0, (cid, direction, setting, "rows that differ", bad.size, bad[:8].tolist())
    _reset(ctx)


# ---- the fall-backs -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid,extra,why", bw.FALLBACKS, ids=[f"{c}-{'-'.join(f'{k}={v}' for k, v in e.items()) or 'as_is'}" for c, e, _ in bw.FALLBACKS])
@pytest.mark.parametrize("values", ["exact", "real"])
def test_fallbacks_run_as_before(da, cid, extra, why, values):
    from helpers import make_ctx
    case = bw.case_by_id(cid)
    _, gname, F, options = case
    g = ar.graph(gname, values)
    variant = extra.get("spmm_variant", 2)
    ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), options=dict(options, **{k: v for k, v in extra.items() if k != "spmm_variant"}))
    for direction in ar.DIRECTIONS:
        ptr, idx, val, _ = ar.side(g, direction)
        x, xg = ar.features(g, direction, F, values == "exact")
        _, _, xl_name, xg_name, _ = _tensors(da, direction)
        ctx.upload(xl_name[0], xl_name[1], x)
        ctx.upload(xg_name[0], xg_name[1], xg)
        rec, form, _ = bw.wide_record(case, direction, extra)
        assert form is None
        _set(ctx, variant, 0)
        off, moved_off = _aggregate(ctx, da, direction)
        _set(ctx, variant, 1)
        on, moved_on = _aggregate(ctx, da, direction)
        assert moved_on[WIDE] == 0, (cid, extra, direction, moved_on)
        assert moved_on == moved_off, (cid, extra, direction, moved_on, moved_off)
        family = {"k1s": K1S, "k1": "spmm_launches_k1"}[rec["family"]]
        assert moved_on[family] == 1 and moved_on[BF_K1S] == (1 if rec["family"] == "k1s" else 0), (cid, extra, direction, why, moved_on)
        assert np.array_equal(_raw(on), _raw(off)), (cid, extra, direction)
        if values == "exact":
            want = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1).astype(np.float32)
            assert np.array_equal(_bits(on), _bits(want)), (cid, extra, direction)
    ctx.close()


# ---- whole epochs -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("epoch_graph", [0, 1])
def test_three_engine_epochs_give_the_same_weights(da, epoch_graph):
    """a graph with a sweep layout (spmm_blk_nb set), gcn_bf16_gather = 2, one dory_engine_run of three epochs: weights, gradients and
    tensors are identical with gcn_bf16_wide on and off; all three aggregations of an epoch are 128 floats or wider and run wide"""
    V, E, dims = 2000, 30000, [602, 128, 41]
    states, wide_runs = [], []
    for wide in (0, 1):
        rng = np.random.default_rng(9)
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        part = da.Partition.build(np.concatenate([s, d]), np.concatenate([d, s]), np.zeros(V, np.int32), 0, 1)
        X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
        labels = rng.integers(0, dims[-1], V).astype(np.uint32)
        ctx = da.Context(0)
        ctx.configure(da.GCN, dims, V)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("gcn_bf16_gather", 2)
        ctx.set_option("gcn_bf16_wide", wide)
        part.upload(ctx)
        ctx.preallocate()
        ctx.weights_init_xavier()
        ctx.adam_config(0.01)
        ctx.upload(0, "x", X)
        ctx.labels_upload(labels)
        ctx.set_option("epoch_graph", epoch_graph)
        eng = da.NativeEngine(ctx)
        eng.run(3)
        if epoch_graph:
            assert ctx.get_option("epoch_graph_recorded") == 1
        wide_runs.append((ctx.get_option(WIDE), ctx.get_option(BF_K1S), ctx.get_option(K1S)))
        st = {}
        for l in range(2):
            st[("w", l)] = ctx.weight_get(l, "w")
            st[("dw", l)] = ctx.weight_grad_get(l, "w")
            st[("ah", l)] = ctx.download(l, "ah")
        st[("h", 0)] = ctx.download(0, "h")
        st[("aTg", 0)] = ctx.download(0, "aTg")
        states.append(st)
        eng.close()
        ctx.close()
    assert wide_runs[0][0] == 0 and wide_runs[0][1] == wide_runs[0][2] > 0, wide_runs
    # eager: three aggregations per epoch; recorded: the eager epochs and the recording count, the replays do not
    assert wide_runs[1][0] == wide_runs[1][1] == wide_runs[1][2] == wide_runs[0][2], wide_runs
    if not epoch_graph:
        assert wide_runs[1][0] == 9, wide_runs
    for k in states[0]:
        assert np.isfinite(states[0][k]).all(), k
        assert np.array_equal(_raw(states[0][k]), _raw(states[1][k])), (epoch_graph, k)


def _golden(da, name):
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


class _Counting:
    """the package with a Context that notes its wide counter when it is closed (run_local closes its contexts itself)"""

    def __init__(self, da, log):
        class Context(da.Context):
            def close(self):
                if self.h:
                    log.append((self.get_option(WIDE), self.get_option(BF_K1S)))
                super().close()
        self._da, self.Context = da, Context

    def __getattr__(self, name):
        return getattr(self._da, name)


@pytest.mark.parametrize("name", ["parts_toy60_p2", "parts_hub3000_p2"])
def test_two_ranks_with_and_without_overlap(da, name):
    """two ranks on the in-process device transport, three epochs, layers of 160 and 128 floats: halo_overlap on and off, gcn_bf16_wide
    on and off -- four runs, the same bits (the ghost rows are converted only once their exchange has landed, whichever form reads
    them)"""
    from local_ranks import run_local
    dims, epochs = [160, 128, 6], 3
    runs, logs = {}, {}
    for wide in (0, 1):
        for overlap in (1, 0):
            pobjs, parts = _golden(da, name)
            assert len(pobjs) == 2
            V, L = len(parts), len(dims) - 1
            rng = np.random.default_rng(5)
            X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
            labels = rng.integers(0, dims[-1], V).astype(np.uint32)
            Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]

            def setup(ctx, r, g):
                if g["localVtxCnt"]:
                    ctx.upload(0, "x", X[g["localToGlobal"]])
                if g["srcGhostCnt"]:
                    ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), dims[0]))
                ctx.labels_upload(labels[g["localToGlobal"]])
                for l, W in enumerate(Ws):
                    ctx.weight_set(l, "w", W)
            dl = [(l, "ah") for l in range(L)] + [(l, nm) for l in range(L - 1) for nm in ("h", "aTg")]
            log = []
            runs[(wide, overlap)] = run_local(_Counting(da, log), pobjs, parts, dims, da.GCN, epochs, setup,
                                              dict(spmm_blk_nb=8, halo_overlap=overlap, gcn_bf16_gather=2, gcn_bf16_wide=wide), downloads=dl)
            logs[(wide, overlap)] = log
    for (wide, overlap), log in logs.items():
        assert len(log) == 2
        for n_wide, n_k1s in log:      # K1s ran on bf16 rows on every rank (all rows here are 128 floats or wider), wide where asked for
            assert 0 < n_k1s <= 3 * epochs and n_wide == (n_k1s if wide else 0), (name, wide, overlap, log)
    a = runs[(0, 1)]
    for key, b in runs.items():
        for r in range(2):
            for k in a["tensors"][r]:
                assert np.array_equal(_raw(a["tensors"][r][k]), _raw(b["tensors"][r][k])), (name, key, r, k)
            for l in range(len(dims) - 1):
                assert np.array_equal(_raw(a["weights"][r][l]["w"]), _raw(b["weights"][r][l]["w"])), (name, key, r, l)
                assert np.array_equal(_raw(a["wgrads"][r][l]["w"]), _raw(b["wgrads"][r][l]["w"])), (name, key, r, l)
