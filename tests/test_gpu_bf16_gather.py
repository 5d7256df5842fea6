"""Option gcn_bf16_gather (include/dorylus_hip.h): GCN aggregations that read their source rows rounded to bf16 (round to
nearest even) and sum in fp32.  1 = the forward aggregations, 2 = the backward ones too.

  * exactness: aggregating X in mode 1 (2) gives, bit for bit, what the fp32 path gives on bf16(X) -- same context, same
    layout, same order of additions; K1s (one and two launches, split hub rows), K1 (plain, local-first edge split, long
    rows); special values (ties, +-0, huge, rounding into the next binade and to +-inf, fp32 subnormals);
  * the error bound against the oracle on unrounded inputs; a 2-layer epoch against an oracle that rounds what it gathers;
  * overlap on / off and epoch-graph replays give the same bits; the planted-communities task is still learned;
  * refusals: GAT contexts, values outside {0, 1, 2}, spmm_variant = 1 (K1b has no bf16 form)."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def bf16(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).to(torch.bfloat16).float().numpy()


def _inputs(rng, rows, F, special=True, finite=False):
    X = rng.standard_normal((rows, F)).astype(np.float32)
    if not special or rows == 0:
        return X
    sp = np.array([1.0 + 2.0 ** -8,                     # tie: rounds to the even neighbour 1.0
                   1.0 + 3 * 2.0 ** -8,                 # tie: rounds up to 1 + 2**-6
                   -(1.0 + 2.0 ** -8), 0.0, -0.0,
                   1e30, -2.5e37, 7.7e-30,
                   np.frombuffer(np.uint32(0x3FFFFFFF).tobytes(), np.float32)[0],   # 1.9999999 -> 2.0 (next binade)
                   np.frombuffer(np.uint32(0x3F7FFFFF).tobytes(), np.float32)[0],   # 0.99999994 -> 1.0
                   3.4e38, -3.4028235e38,               # round to +inf / -inf
                   1e-40, -3e-39, 2.0 ** -133, 1.1754942e-38],                       # fp32 subnormals
                  np.float32)
    if finite:
        sp = sp[np.isfinite(bf16(sp))]
    n = min(rows, 48)
    rr = rng.choice(rows, n, replace=False)
    for i, r in enumerate(rr):
        X[r, rng.integers(0, F, 3)] = sp[(i + np.arange(3)) % sp.size]
    # one column of fp32 subnormals on every row: bf16 keeps them (nearest even, as torch rounds), the fp32 sums see them
    X[:, 1 % F] = (rng.uniform(0.5, 1.5, rows) * 1e-39 * rng.choice([-1, 1], rows)).astype(np.float32)
    return X


STEPS = {"f0": ((0, "x"), (0, "fg")), "f1": ((0, "h"), (1, "fg")), "b1": ((1, "grad"), (0, "bg"))}


def _run_step(ctx, da, st):
    if st == "f0":
        ctx.aggregate(0, da.FORWARD)
        return ctx.download(0, "ah")
    if st == "f1":
        ctx.aggregate(1, da.FORWARD)
        return ctx.download(1, "ah")
    ctx.aggregate(1, da.BACKWARD)
    return ctx.download(0, "aTg")


def _upload(ctx, ins, st, rounded):
    for key in STEPS[st]:
        if key in ins and ins[key].shape[0]:
            ctx.upload(key[0], key[1], bf16(ins[key]) if rounded else ins[key])


def _counters(ctx):
    return ctx.get_option("gcn_bf16_gathers_k1s"), ctx.get_option("gcn_bf16_gathers_k1")


def _check_exact(ctx, da, ins, variant, what):
    """every aggregation step in modes 1 and 2 against mode 0 on the rounded inputs; returns the kernel families that ran"""
    fams = []
    for mode in (1, 2):
        for st in STEPS:
            rounded = st != "b1" or mode == 2
            ctx.set_option("spmm_variant", variant)
            ctx.set_option("gcn_bf16_gather", mode)
            _upload(ctx, ins, st, False)
            c0 = _counters(ctx)
            got = _run_step(ctx, da, st)
            c1 = _counters(ctx)
            d_k1s, d_k1 = c1[0] - c0[0], c1[1] - c0[1]
            assert d_k1s + d_k1 == (1 if rounded else 0), (what, mode, st, c0, c1)
            # where the fp32 path would take K1b (variant 2 without a sweep layout), bf16 runs K1: compare against K1
            ref_variant = 0 if d_k1 else variant
            ctx.set_option("gcn_bf16_gather", 0)
            ctx.set_option("spmm_variant", ref_variant)
            _upload(ctx, ins, st, rounded)
            ref = _run_step(ctx, da, st)
            assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (what, mode, st, variant, ref_variant)
            if st == "f0":      # (the subnormal column: kept by the conversion, so the sums are not all zero)
                assert np.count_nonzero(got[:, 1]) > 0.5 * got.shape[0], (what, mode)
            fams.append("k1s" if d_k1s else ("k1" if d_k1 else "fp32"))
    return fams


def _graph(seed, V, E, hub=False):
    from helpers import random_graph
    s, d = random_graph(seed, V, E)
    if hub:      # one destination and one source far beyond K1's row clamp (8192 edges) and the sweep's split degree
        rng = np.random.default_rng(seed + 1)
        s = np.concatenate([s, rng.integers(0, V, 12000).astype(np.uint32), np.full(10000, 11, np.uint32)])
        d = np.concatenate([d, np.full(12000, 7, np.uint32), rng.integers(0, V, 10000).astype(np.uint32)])
    return s, d


def _ctx_inputs(rng, g, F, special=True, finite=False):
    N, Gs, Gd = int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
    return {(0, "x"): _inputs(rng, N, F, special, finite), (0, "fg"): _inputs(rng, Gs, F, special, finite),
            (0, "h"): _inputs(rng, N, F, special, finite), (1, "fg"): _inputs(rng, Gs, F, special, finite),
            (1, "grad"): _inputs(rng, N, F, special, finite), (0, "bg"): _inputs(rng, Gd, F, special, finite)}


@pytest.mark.parametrize("F", [16, 41, 128, 602])
def test_k1s_bf16_rows_equal_fp32_on_rounded_rows(da, F):
    import partition_oracle as po
    from helpers import make_ctx
    V = 20000
    s, d = _graph(1, V, 120000)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    ctx = make_ctx(da, g, [F, F, 3], V)
    ins = _ctx_inputs(np.random.default_rng(F), g, F)
    fams = _check_exact(ctx, da, ins, 2, ("k1s", F))
    assert fams == ["k1s", "k1s", "fp32", "k1s", "k1s", "k1s"], fams
    fams = _check_exact(ctx, da, ins, 0, ("k1", F))
    assert fams == ["k1", "k1", "fp32", "k1", "k1", "k1"], fams
    ctx.close()


@pytest.mark.parametrize("F", [41, 128])
def test_hub_rows_bf16(da, F):
    """rows far beyond the sweep's split degree (pieces + combine kernel) and beyond K1's row clamp (long-row kernels)"""
    import partition_oracle as po
    from helpers import make_ctx
    V = 20000
    s, d = _graph(2, V, 120000, hub=True)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    assert np.diff(g["colPtr"].astype(np.int64)).max() > 8192 and np.diff(g["rowPtr"].astype(np.int64)).max() > 8192
    ctx = make_ctx(da, g, [F, F, 3], V)
    ins = _ctx_inputs(np.random.default_rng(F + 7), g, F)
    fams = [f for f in _check_exact(ctx, da, ins, 2, ("hub", F)) if f != "fp32"]
    assert set(fams) <= {"k1s", "k1"}, fams
    assert _check_exact(ctx, da, ins, 0, ("hub k1", F)).count("k1") == 5
    ctx.close()


@pytest.mark.parametrize("F", [41, 602])
def test_ghost_rows_bf16(da, F):
    """a partition with ghost rows uploaded as fg@0 / fg@1 / bg@0: K1s in two launches (local-source blocks, then the ghost
    blocks), K1 with the local-first edge split (spmm_blk_force_split: what runs beside an exchange in flight)"""
    from helpers import make_ctx, partitions
    V = 40000
    s, d = _graph(3, V, 240000)
    parts = np.random.default_rng(3).integers(0, 2, V)
    gs = partitions(s, d, parts, 2)
    for r, g in enumerate(gs):
        assert g["srcGhostCnt"] > 0 and g["dstGhostCnt"] > 0
        ctx = make_ctx(da, g, [F, F, 3], V, node_id=r, num_nodes=2)
        ins = _ctx_inputs(np.random.default_rng(F + r), g, F)
        assert _check_exact(ctx, da, ins, 2, ("ghost k1s", r, F)).count("k1s") == 5
        ctx.set_option("spmm_blk_force_split", 1)
        assert _check_exact(ctx, da, ins, 0, ("ghost k1 split", r, F)).count("k1") == 5
        ctx.close()


@pytest.mark.parametrize("nb", [0, 8])
def test_error_bound_against_oracle_reddit_dims(da, golden_dir, nb):
    """per element |bf16 path - oracle on unrounded fp32| <= 2**-8 S + 1e-6 S, S = sum |w| |x| + |norm_v| |x_v|; the
    Reddit-dims fixture's graph and widths (602 forward, 128 backward), K1 (nb = 0) and K1s (nb = 8).  bf16 subnormals are
    spaced 2**-133 apart whatever their size, so an fp32 subnormal rounds with an ABSOLUTE error of up to 2**-134: the bound
    carries 2**-133 W, W = sum |w| + |norm_v| (measured: a column of fp32 subnormals exceeds the relative bound alone 1.54x)"""
    import orc
    import partition_oracle as po
    from helpers import make_ctx
    z = np.load(os.path.join(golden_dir, "numpy_gnn_reddit_dims.npz"))
    V = int(z["V"])
    dims = [int(x) for x in z["dims"]]
    g = po.preprocess(z["src"].astype(np.uint32), z["dst"].astype(np.uint32), np.zeros(V, np.int64), 0, 1)
    ctx = make_ctx(da, g, dims, V, options={"spmm_blk_nb": nb} if nb else None)
    ctx.set_option("gcn_bf16_gather", 2)
    rng = np.random.default_rng(11)
    X = _inputs(rng, V, dims[0], finite=True) * np.float32(3)
    H = _inputs(rng, V, dims[1], finite=True)
    Gr = _inputs(rng, V, dims[1], finite=True)
    ctx.upload(0, "x", X); ctx.upload(0, "h", H); ctx.upload(1, "grad", Gr)
    c0 = _counters(ctx)
    got = [_run_step(ctx, da, st) for st in ("f0", "f1", "b1")]
    c1 = _counters(ctx)
    assert (c1[0] - c0[0] == 3) if nb else (c1[1] - c0[1] == 3), (c0, c1)
    e0 = np.zeros((0, 1), np.float32)
    for (ptr, idx, val), x, y in (((g["colPtr"], g["rowIdx"], g["cscVal"]), X, got[0]),
                                  ((g["colPtr"], g["rowIdx"], g["cscVal"]), H, got[1]),
                                  ((g["rowPtr"], g["colIdx"], g["csrVal"]), Gr, got[2])):
        ref = orc.aggregate_gcn(ptr, idx, val, g["norm"], x, e0.reshape(0, x.shape[1]))
        S = orc.aggregate_gcn(ptr, idx, np.abs(val), np.abs(g["norm"]), np.abs(x), e0.reshape(0, x.shape[1]))
        W = orc.aggregate_gcn(ptr, idx, np.abs(val), np.abs(g["norm"]), np.ones_like(x), e0.reshape(0, x.shape[1]))
        err = np.abs(y.astype(np.float64) - ref)
        bound = (2.0 ** -8 + 1e-6) * S.astype(np.float64) + 2.0 ** -133 * W.astype(np.float64)
        assert np.all(err <= bound), float((err / np.maximum(bound, 1e-300)).max())
        assert err.max() > 0          # (the rounding is really there)
    ctx.close()


# ---- a 2-layer epoch against the oracle sequence of helpers.oracle_gcn_epoch, with the gathered inputs rounded ----------
def _round_like(ref, gpu):
    """bf16(ref), except where the oracle's and the GPU's fp32 values agree to the parity criterion (1e-4 relative) but
    straddle a bf16 rounding boundary: there the GPU's rounding is taken (a one-ulp bf16 flip from fp32 noise is not
    an error of the path).  Such elements must be rare."""
    rb, gb = bf16(ref), bf16(gpu)
    amb = (rb != gb) & (np.abs(ref - gpu) <= 1e-4 * np.abs(ref) + 1e-30)
    assert amb.sum() <= max(8, 1e-3 * ref.size), int(amb.sum())
    return np.where(amb, gb, rb).astype(np.float32)


def _oracle_bf16_epoch(g, X, labels, Ws, V, mode, gpu):
    import orc
    N = X.shape[0]
    T = {}
    T["ah0"] = orc.aggregate_gcn(g["colPtr"], g["rowIdx"], g["cscVal"], g["norm"], bf16(X), np.zeros((0, X.shape[1]), np.float32))
    T["z0"], T["h0"] = orc.vtx_forward_hidden(T["ah0"], Ws[0])
    hb = _round_like(T["h0"], gpu["h0"])
    T["ah1"] = orc.aggregate_gcn(g["colPtr"], g["rowIdx"], g["cscVal"], g["norm"], hb, np.zeros((0, hb.shape[1]), np.float32))
    C = Ws[1].shape[1]
    lab = np.eye(C, dtype=np.float32)[labels[:N]]
    res = orc.vtx_forward_last(T["ah1"], Ws[1], lab, V)
    T["grad1"] = res["grad"]
    dW1 = res["dW"]
    gb = _round_like(res["grad"], gpu["grad1"]) if mode == 2 else res["grad"]
    T["aTg0"] = orc.aggregate_gcn(g["rowPtr"], g["colIdx"], g["csrVal"], g["norm"], gb, np.zeros((0, gb.shape[1]), np.float32))
    _, dW0, _ = orc.vtx_backward(T["aTg0"], T["z0"], T["ah0"], Ws[0], 0)
    return T, [dW0, dW1]


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("nb", [0, 8])
def test_epoch_parity_with_rounded_gathers(da, mode, nb):
    from helpers import assert_parity, rel_err
    V, E, dims = 2000, 30000, [602, 128, 41]
    rng = np.random.default_rng(mode)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    src, dst = np.concatenate([s, d]), np.concatenate([d, s])
    part = da.Partition.build(src, dst, np.zeros(V, np.int32), 0, 1)
    g = part.view()
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    ctx = da.Context(0)
    ctx.configure(da.GCN, dims, V)
    if nb:
        ctx.set_option("spmm_blk_nb", nb)
    ctx.set_option("gcn_bf16_gather", mode)
    part.upload(ctx)
    ctx.preallocate()
    ctx.weights_init_xavier()
    Ws = [ctx.weight_get(0), ctx.weight_get(1)]
    ctx.upload(0, "x", X)
    ctx.labels_upload(labels)
    c0 = _counters(ctx)
    eng = da.NativeEngine(ctx)
    eng.run(1)
    c1 = _counters(ctx)
    assert (c1[0] - c0[0] if nb else c1[1] - c0[1]) == (2 if mode == 1 else 3), (c0, c1)
    gpu = {"h0": ctx.download(0, "h"), "grad1": ctx.download(1, "grad")}
    T, dW = _oracle_bf16_epoch(g, X, labels, Ws, V, mode, gpu)
    assert_parity(ctx.download(0, "ah"), T["ah0"], "ah0")
    assert_parity(gpu["h0"], T["h0"], "h0")
    assert_parity(ctx.download(1, "ah"), T["ah1"], "ah1")
    assert_parity(ctx.download(0, "aTg"), T["aTg0"], "aTg0")
    assert rel_err(ctx.weight_grad_get(0), dW[0]) < 1e-4 and rel_err(ctx.weight_grad_get(1), dW[1]) < 1e-4
    eng.close()
    ctx.close()


# ---- overlap, epoch graph -----------------------------------------------------------------------------------------------
def _golden(da, name):
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy60_p4_hash"])
def test_overlap_on_and_off_give_the_same_bits(da, case):
    """P ranks on the in-process device transport, mode 2: the ghost rows are converted only after their exchange has
    landed, so overlapping the local-source launches with the exchange changes no bit"""
    from local_ranks import run_local
    dims, epochs = [20, 16, 6], 3
    for opts in ({"spmm_blk_nb": 8}, {"spmm_variant": 0}):
        runs = []
        for overlap in (1, 0):
            pobjs, parts = _golden(da, case)
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
            runs.append(run_local(da, pobjs, parts, dims, da.GCN, epochs, setup,
                                  dict(opts, halo_overlap=overlap, gcn_bf16_gather=2), downloads=dl))
        a, b = runs
        assert len(a["tensors"]) == len(pobjs) >= 2
        for r in range(len(a["tensors"])):
            for k in a["tensors"][r]:
                assert np.array_equal(a["tensors"][r][k], b["tensors"][r][k]), (case, opts, r, k)
            for l in range(L):
                assert np.array_equal(a["weights"][r][l]["w"], b["weights"][r][l]["w"]), (case, opts, r, l)
                assert np.array_equal(a["wgrads"][r][l]["w"], b["wgrads"][r][l]["w"]), (case, opts, r, l)


@pytest.mark.parametrize("nb", [0, 8])
def test_replayed_bf16_epochs_are_bit_identical_to_eager(da, nb):
    import partition_oracle as po
    V, E, dims = 2708, 5278, [1433, 16, 7]
    states = []
    for graph in (0, 1):
        rng = np.random.default_rng(5)
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
        g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
        ctx = da.Context(0)
        ctx.configure(da.GCN, dims, V)
        if nb:
            ctx.set_option("spmm_blk_nb", nb)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.fill_uniform(0, "x", 3, -1.0, 1.0, g["localToGlobal"])
        ctx.labels_upload(rng.integers(0, dims[-1], V).astype(np.uint32))
        ctx.weights_init_xavier()
        ctx.adam_config(0.01)
        ctx.set_option("gcn_bf16_gather", 2)
        ctx.set_option("epoch_graph", graph)
        c0 = _counters(ctx)
        eng = da.NativeEngine(ctx)
        eng.run(6)
        eng.run(4)
        c1 = _counters(ctx)
        assert sum(c1) > sum(c0)
        if graph:
            assert ctx.get_option("epoch_graph_recorded") == 1
        st = {}
        for l in range(2):
            st[("w", l)] = ctx.weight_get(l, "w")
            st[("dw", l)] = ctx.weight_grad_get(l, "w")
            for nm in ("ah", "z", "g"):
                st[(nm, l)] = ctx.download(l, nm)
        st[("h", 0)] = ctx.download(0, "h")
        st[("aTg", 0)] = ctx.download(0, "aTg")
        states.append(st)
        eng.close()
        ctx.close()
    for k in states[0]:
        assert np.array_equal(states[0][k], states[1][k]), k


# ---- it still learns ------------------------------------------------------------------------------------------------------
def _task(V=6000, C=6, deg=12, F=24, seed=4):
    rng = np.random.default_rng(seed)
    y = rng.integers(0, C, V)
    members = [np.nonzero(y == c)[0] for c in range(C)]
    s = rng.integers(0, V, V * deg // 2)
    same = rng.random(s.size) < 0.8
    d = np.where(same, [members[y[v]][rng.integers(0, members[y[v]].size)] for v in s], rng.integers(0, V, s.size))
    s, d = np.concatenate([s, d]), np.concatenate([d, s])
    X = rng.standard_normal((V, F)).astype(np.float32)
    X[np.arange(V), y] += 1.0
    return s.astype(np.uint32), d.astype(np.uint32), X, y.astype(np.uint32), C


@pytest.mark.parametrize("mode", [1, 2])
def test_planted_communities_are_learned_with_bf16_rows(da, mode):
    s, d, X, y, C = _task()
    V, F = X.shape
    part = da.Partition.build(s, d, np.zeros(V, np.int32), 0, 1)
    ctx = da.Context(0)
    ctx.configure(da.GCN, [F, 16, C], V)
    ctx.set_option("gcn_bf16_gather", mode)
    part.upload(ctx)
    ctx.preallocate()
    ctx.upload(0, "x", X)
    ctx.labels_upload(y)
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    eng = da.NativeEngine(ctx)
    acc = []
    for _ in range(12):
        eng.run(5)
        a, l, n = ctx.train_stat()
        acc.append(a / n)
    assert sum(_counters(ctx)) >= 60 * (2 if mode == 1 else 3)
    eng.close()
    ctx.close()
    assert acc[-1] > 0.85 and acc[-1] > acc[0], acc


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals(da):
    import partition_oracle as po
    for gnn in (da.GAT, da.GATMH):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        with pytest.raises(da.DoryError):
            ctx.set_option("gcn_bf16_gather", 1)
        ctx.set_option("gcn_bf16_gather", 0)
        assert ctx.get_option("gcn_bf16_gather") == 0
        ctx.close()
    ctx = da.Context(0)                       # set on a fresh context, then configured as GAT: refused there
    ctx.set_option("gcn_bf16_gather", 1)
    with pytest.raises(da.DoryError):
        ctx.configure(da.GAT, [16, 8, 3], 100)
    ctx.close()
    V = 300
    rng = np.random.default_rng(0)
    s, d = rng.integers(0, V, 900), rng.integers(0, V, 900)
    g = po.preprocess(np.concatenate([s, d]), np.concatenate([d, s]), np.zeros(V, np.int64), 0, 1)
    from helpers import make_ctx
    ctx = make_ctx(da, g, [64, 32, 3], V)
    for bad in (3, -1, 100):
        with pytest.raises(da.DoryError):
            ctx.set_option("gcn_bf16_gather", bad)
    assert ctx.get_option("gcn_bf16_gather") == 0
    ctx.upload(0, "x", rng.standard_normal((V, 64)).astype(np.float32))
    ctx.set_option("spmm_variant", 1)
    ctx.set_option("gcn_bf16_gather", 1)
    with pytest.raises(da.DoryError, match="spmm_variant"):
        ctx.aggregate(0, da.FORWARD)
    ctx.set_option("gcn_bf16_gather", 0)
    ctx.aggregate(0, da.FORWARD)             # (fp32 K1b as before)
    ctx.close()
