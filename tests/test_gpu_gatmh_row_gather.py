"""The multi-head GAT's row-gather kernels with ghost rows (csrc/gat_mh_rows.hip; dory_gatmh_row_gather): the family a partitioned
dory_aggregate runs where neither the sweep layout nor the source-blocked layout applies (mode 0, the default), and everywhere with
mode 1.  Every comparison is against oracle/gat_mh_oracle.py (float64), with the tolerances of tests/test_gpu_gat_mh.py."""
import glob
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RTOL = 1e-4
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FWD, EDGE, ROWWISE, SRC = 0, 1, 2, 3       # dory_gatmh_row_gather_stats


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def _params(rng, dims, heads, scale=0.3):
    out = []
    for l in range(2):
        zw = dims[l + 1] * (heads[l] if l == 1 else 1)
        out.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                    (rng.standard_normal(zw) * scale).astype(np.float32), (rng.standard_normal(zw) * scale).astype(np.float32)])
    return out


def _pad_ld(cols):
    return cols if cols <= 1 else (cols + 31) // 32 * 32


def _dst_rowwise_covers(K, zw):
    """gatmh_sweep_hl(K, D, ld) != 0 and (ld / 4) % HL == 0, restated: the shapes launch_gatmh_dst_rowwise takes"""
    D, ld = zw // K, _pad_ld(zw)
    group = 32 if ld >= 128 else 16
    if K == 1:
        hl = 16 if (ld <= 64 and group == 16) else 0
    elif D % 4 or D & (D - 1):
        hl = 0
    else:
        hl = D // 4 if 2 <= D // 4 <= min(16, group) else 0
    return hl != 0 and (ld // 4) % hl == 0


def _layer_shapes(dims, heads):
    return [(heads[l], dims[l + 1] * (heads[l] if l == 1 else 1)) for l in range(2)]     # (K, z width) per layer


def _hub_graph(P, V=240, E=2600):
    """the graph of test_gat_mh_partitioned_epoch_vs_oracle: a hub destination of 200 in-edges, a hub source of 200 out-edges,
    scattered ownership"""
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % P).astype(np.int64)
    return s, d, parts, rng


def _partitioned(da, gs, parts, X, labels, params, dims, heads, opts, mode):
    """One epoch over P contexts, the ghost rows moved by halo_pack_tensor / halo_unpack_tensor and a device copy, the backward in
    its phases 1 / 2.  Returns ({(layer, name): rows in global order}, summed weight gradients per layer, the counters of every
    rank after each layer's backward: stats[rank][layer], and at the end: stats[rank][None])."""
    import torch
    from halo_plan_ref import halo_plan
    P, V, L = len(gs), len(parts), 2
    ctxs, plans = [], []
    for r, g in enumerate(gs):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V, r, P)
        ctx.gatmh_heads(heads)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.gatmh_row_gather(mode)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        pl = halo_plan(g, parts, r, P)
        for dd in (0, 1):
            ctx.halo_plan(dd, pl[dd][0], pl[dd][1])
        ctxs.append(ctx)
        plans.append(pl)

    def exchange(layer, src_name, ghost_name, dd):
        if P == 1:
            return
        _, _, ld, _ = ctxs[0].info(layer, src_name)
        send = [torch.zeros(max(1, sum(len(x) for x in plans[r][dd][0])) * ld, device="cuda") for r in range(P)]
        recv = [torch.zeros(max(1, sum(len(x) for x in plans[r][dd][1])) * ld, device="cuda") for r in range(P)]
        torch.cuda.synchronize()   # (the contexts' streams are non-blocking: torch's zero fills must have landed before a pack kernel writes)
        for r in range(P):
            ctxs[r].halo_pack_tensor(layer, src_name, dd, send[r].data_ptr())
            ctxs[r].sync()
        for r in range(P):
            soff = np.concatenate([[0], np.cumsum([len(x) for x in plans[r][dd][0]])])
            for p in range(P):
                roff = np.concatenate([[0], np.cumsum([len(x) for x in plans[p][dd][1]])])
                n = len(plans[r][dd][0][p])
                recv[p][roff[r] * ld:(roff[r] + n) * ld] = send[r][soff[p] * ld:(soff[p] + n) * ld]
        torch.cuda.synchronize()
        for r in range(P):
            ctxs[r].halo_unpack_tensor(layer, ghost_name, dd, recv[r].data_ptr())
            ctxs[r].sync()

    stats = [dict() for _ in range(P)]
    try:
        for l in range(L):
            for c in ctxs:
                c.apply_vertex(l, da.FORWARD)
            exchange(l, "z", "fg_z", da.FORWARD)
            for c in ctxs:
                c.apply_edge(l + 1, da.FORWARD)
                c.aggregate(l + 1, da.FORWARD)
        for c in ctxs:
            c.predict_gat(L)
        for l in range(L - 1, -1, -1):
            before = [c.gatmh_row_gather_stats() for c in ctxs]
            for c in ctxs:
                c.set_option("gatmh_bwd_phase", 1)
                c.aggregate(l + 1, da.BACKWARD)
            exchange(l, "do", "bg_do", da.BACKWARD)
            exchange(l, "st", "bg_st", da.BACKWARD)
            for c in ctxs:
                c.set_option("gatmh_bwd_phase", 2)
                c.aggregate(l + 1, da.BACKWARD)
                c.apply_vertex(l, da.BACKWARD)
            for r, c in enumerate(ctxs):
                stats[r][l] = tuple(a - b for a, b in zip(c.gatmh_row_gather_stats(), before[r]))
        T = {}
        names = [(l, nm) for l in range(L) for nm in ("z", "el", "er", "o", "m", "den", "t", "del", "der", "dz")]
        for (l, nm) in names + [(1, "logits"), (1, "grad"), (1, "h")]:
            out = None
            for r, g in enumerate(gs):
                t = ctxs[r].download(l, nm)
                if out is None:
                    out = np.zeros((V, t.shape[1]), np.float32)
                out[g["localToGlobal"]] = t
            T[(l, nm)] = out
        dW = [{nm: sum(c.weight_grad_get(l, nm) for c in ctxs) for nm in ("w", "a_l", "a_r")} for l in range(L)]
        for r, c in enumerate(ctxs):
            stats[r][None] = c.gatmh_row_gather_stats()
    finally:
        for c in ctxs:
            c.close()
    return T, dW, stats


def _check(T, dW, ref, what=(), true_max=True):
    """every tensor, log-sum-exp and weight gradient, as tests/test_gpu_gat_mh.py::_epoch_vs_oracle asserts them"""
    from helpers import rel_err
    fws, Hs, loss, dlogits, grads = ref
    for l in range(2):
        for nm, want in (("z", fws[l]["Z"]), ("el", fws[l]["el"]), ("er", fws[l]["er"]), ("o", fws[l]["O"])):
            e = rel_err(T[(l, nm)], want)
            print(what, l, nm, e)
            assert e < RTOL, (what, l, nm, e)
        for nm, want in (("t", grads[l]["t"]), ("del", grads[l]["d_el"]), ("der", grads[l]["d_er"]), ("dz", grads[l]["dZ"])):
            e = rel_err(T[(l, nm)], want)
            print(what, l, nm, e)
            assert e < 5e-4, (what, l, nm, e)
        for nm, key in (("w", "dW"), ("a_l", "da_l"), ("a_r", "da_r")):
            e = rel_err(np.asarray(dW[l][nm]).reshape(np.shape(grads[l][key])), grads[l][key])
            print(what, l, "d" + nm, e)
            assert e < 5e-4, (what, l, nm, e)
        lse = np.log(T[(l, "den")].astype(np.float64)) + T[(l, "m")]
        e = np.abs(lse - (np.log(fws[l]["den"]) + fws[l]["m"])).max()
        print(what, l, "log-sum-exp", e)
        assert e < 1e-4, (what, l, "log-sum-exp", e)
        # m is the row's TRUE maximum per head (as in the blocked forms)
        assert not true_max or np.abs(T[(l, "m")] - fws[l]["m"]).max() < 1e-4 * max(1.0, np.abs(fws[l]["m"]).max()), (what, l, "m")
    for key, want in (((1, "logits"), Hs[2]), ((1, "grad"), dlogits), ((1, "h"), Hs[1])):
        e = rel_err(T[key], want)
        print(what, key, e)
        assert e < RTOL, (what, key, e)


def _oracle(g_all, X, labels, params, heads):
    import gat_mh_oracle as go
    return go.epoch(g_all, X, labels, [[p.astype(np.float64) for p in ps] for ps in params], heads)


def _hub_case(da, P, dims, heads, opts, mode):
    import partition_oracle as po
    s, d, parts, rng = _hub_graph(P)
    V = len(parts)
    g_all = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    gs = [po.preprocess(s, d, parts, r, P) for r in range(P)]
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = _params(rng, dims, heads)
    T, dW, stats = _partitioned(da, gs, parts, X, labels, params, dims, heads, opts, mode)
    return T, dW, stats, (g_all, X, labels, params), gs


# ---- 1. partitioned epochs, default mode, where no layout is available ------------------------------------------------------------
@pytest.mark.parametrize("dims,heads", [([24, 64, 6], [4, 1]), ([24, 128, 6], [8, 1]), ([24, 256, 6], [4, 1]), ([24, 256, 9], [32, 1]),
                                        ([12, 100, 6], [1, 1]), ([24, 32, 8], [4, 2])])
@pytest.mark.parametrize("P", [2, 4])
def test_partitioned_epoch_vs_oracle_without_layouts(da, P, dims, heads):
    """gatmh_sweep = 0, gatmh_blocked = 0: a partitioned dory_aggregate used to be refused here (DoryError)"""
    T, dW, stats, inp, gs = _hub_case(da, P, dims, heads, {"gatmh_sweep": 0, "gatmh_blocked": 0}, 0)
    _check(T, dW, _oracle(*inp, heads), (P, dims, heads))
    for r, g in enumerate(gs):
        if g["localVtxCnt"]:
            st = stats[r][None]
            assert st[FWD] == 2 and st[SRC] == 2 and st[EDGE] + st[ROWWISE] == 2, (r, st)


# ---- 2. head shapes no layout covers, default options -------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,heads", [([24, 64, 6], [32, 1]), ([16, 32, 5], [32, 1])], ids=["32x2", "32x1"])
def test_head_shapes_no_layout_covers(da, dims, heads):
    T, dW, stats, inp, gs = _hub_case(da, 2, dims, heads, {}, 0)
    _check(T, dW, _oracle(*inp, heads), (dims, heads))
    for r in range(2):
        assert stats[r][0][EDGE] == 1 and stats[r][0][ROWWISE] == 0 and stats[r][0][SRC] == 1, (r, stats[r])   # the 32-head layer
        assert stats[r][None][FWD] >= 1, (r, stats[r])


# ---- 3. forced mode, single partition, through the Engine ---------------------------------------------------------------------------
def _single(da, g, X, labels, params, dims, heads, opts, mode=1):
    """one epoch inside the Engine; (tensors, weight gradients, counters)"""
    V = X.shape[0]
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, V)
    ctx.gatmh_heads(heads)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.gatmh_row_gather(mode)
    ctx.graph_upload(g)
    ctx.preallocate()
    ctx.upload(0, "h", X)
    ctx.labels_upload(labels)
    for l, (W, al, ar) in enumerate(params):
        ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
    ctx.adam_config(0.01)
    eng = da.NativeEngine(ctx)
    try:
        eng.run(1)
        names = [(l, nm) for l in range(2) for nm in ("z", "el", "er", "o", "m", "den", "t", "del", "der", "dz")]
        T = {k: ctx.download(*k) for k in names + [(1, "logits"), (1, "grad"), (1, "h")]}
        dW = [{nm: ctx.weight_grad_get(l, nm) for nm in ("w", "a_l", "a_r")} for l in range(2)]
        stats = ctx.gatmh_row_gather_stats()
        for l in range(2):       # every parameter took an Adam step
            for nm, p in zip(("w", "a_l", "a_r"), params[l]):
                assert not np.array_equal(ctx.weight_get(l, nm).reshape(p.shape), p)
    finally:
        eng.close()
        ctx.close()
    return T, dW, stats


@pytest.mark.parametrize("dims,heads,V,E", [
    ([24, 32, 8], [4, 2], 200, 1500), ([40, 128, 41], [8, 1], 300, 4000), ([16, 64, 7], [1, 1], 150, 900), ([20, 128, 5], [4, 1], 180, 1300),
    ([12, 100, 6], [1, 1], 160, 1100), ([24, 256, 6], [4, 1], 170, 1200), ([24, 256, 9], [32, 1], 140, 1000)])
def test_forced_single_partition_epoch_vs_oracle(da, dims, heads, V, E):
    import partition_oracle as po
    rng = np.random.default_rng(len(dims) + V)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    s[:40], d[:40] = 3, rng.integers(0, V, 40)            # a hub source
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = _params(rng, dims, heads)
    T, dW, stats = _single(da, g, X, labels, params, dims, heads, {})
    _check(T, dW, _oracle(g, X, labels, params, heads), (dims, heads))
    covered = sum(_dst_rowwise_covers(K, zw) for K, zw in _layer_shapes(dims, heads))
    assert stats == (2, 2 - covered, covered, 2), (stats, covered)
    # the forward forms the sources' scores from the gathered rows with the arithmetic of the kernel that wrote "el": m, the row's
    # true maximum, is then the maximum of LeakyReLU(el[u] + er[v]) over the tensors' own values, to the bit
    src = np.concatenate([np.asarray(g["rowIdx"], np.int64), np.arange(V)])
    dst = np.concatenate([np.repeat(np.arange(V), np.diff(np.asarray(g["colPtr"], np.int64))), np.arange(V)])
    for l in range(2):
        K = heads[l]
        pre = T[(l, "el")][src, :K] + T[(l, "er")][dst, :K]
        sc = np.where(pre > 0, pre, np.float32(0.2) * pre).astype(np.float32)
        want = np.full((V, K), -np.inf, np.float32)
        np.maximum.at(want, dst, sc)
        assert np.array_equal(T[(l, "m")][:, :K], want), (l, np.abs(T[(l, "m")][:, :K] - want).max())


@pytest.mark.parametrize("dims,heads", [([24, 96, 6], [3, 1]), ([24, 160, 5], [5, 1]), ([12, 80, 6], [1, 1]), ([24, 224, 6], [7, 1])],
                         ids=["3x32", "5x32", "1x80", "7x32"])
def test_rows_whose_float4_count_is_no_power_of_two(da, dims, heads):
    """ld = 96, 160, 96, 224: 32- and 64-lane groups with idle lanes, the forms that gather el instead of forming it from the row;
    two ranks, mode 1"""
    T, dW, stats, inp, gs = _hub_case(da, 2, dims, heads, {}, 1)
    _check(T, dW, _oracle(*inp, heads), (dims, heads))
    for r in range(2):
        assert stats[r][None][FWD] == 2 and stats[r][None][SRC] == 2, (r, stats[r])


# ---- 4. the edges of the row walk ------------------------------------------------------------------------------------------------------
DIMS8, HEADS8 = [24, 128, 6], [8, 1]


@pytest.mark.parametrize("N", [5, 67])
def test_rows_without_edges_and_odd_row_counts(da, N):
    """N is no multiple of any rows-per-block (4 .. 32); vertex 0 has no in-edges (o = z, den = 1), vertex 1 no out-edges"""
    import partition_oracle as po
    rng = np.random.default_rng(N)
    E = 6 * N
    s, d = rng.integers(1, N, E), rng.integers(1, N, E)
    s[s == 1] = 2                                           # 1 is never a source, 0 never a destination
    s[:3] = 0                                               # (0 has out-edges)
    g = po.preprocess(s, d, np.zeros(N, np.int64), 0, 1)
    assert g["colPtr"][1] == g["colPtr"][0] and g["rowPtr"][2] == g["rowPtr"][1]
    X = rng.uniform(-1, 1, (N, DIMS8[0])).astype(np.float32)
    labels = rng.integers(0, DIMS8[-1], N).astype(np.uint32)
    params = _params(rng, DIMS8, HEADS8)
    T, dW, stats = _single(da, g, X, labels, params, DIMS8, HEADS8, {})
    _check(T, dW, _oracle(g, X, labels, params, HEADS8), ("N", N))
    for l in range(2):
        assert np.array_equal(T[(l, "o")][0], T[(l, "z")][0]), l
        assert np.all(T[(l, "den")][0] == 1.0), l


def _two_rank_case(da, s, d, parts, seed):
    import partition_oracle as po
    V = len(parts)
    rng = np.random.default_rng(seed)
    g_all = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
    X = rng.uniform(-1, 1, (V, DIMS8[0])).astype(np.float32)
    labels = rng.integers(0, DIMS8[-1], V).astype(np.uint32)
    params = _params(rng, DIMS8, HEADS8)
    T, dW, stats = _partitioned(da, gs, parts, X, labels, params, DIMS8, HEADS8, {}, 1)
    _check(T, dW, _oracle(g_all, X, labels, params, HEADS8), ("two ranks", seed))
    return gs, stats


def test_a_rank_that_owns_nothing(da):
    rng = np.random.default_rng(3)
    V, E = 60, 500
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    gs, stats = _two_rank_case(da, s, d, np.zeros(V, np.int64), 3)
    assert gs[1]["localVtxCnt"] == 0
    assert stats[0][None] == (2, 1, 1, 2) and stats[1][None] == (0, 0, 0, 0), stats      # (the last layer, one head of 6: an edge pass)


def test_ghosts_on_one_side_only(da):
    """every cross edge runs from rank 0 to rank 1: rank 0 has ghost destinations and no ghost sources (a null fg_z), rank 1 the reverse"""
    rng = np.random.default_rng(4)
    V, E = 80, 700
    parts = (np.arange(V) >= 40).astype(np.int64)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    back = (parts[s] == 1) & (parts[d] == 0)
    d[back] = rng.integers(40, V, int(back.sum()))
    gs, stats = _two_rank_case(da, s, d, parts, 4)
    assert gs[0]["srcGhostCnt"] == 0 and gs[0]["dstGhostCnt"] > 0 and gs[1]["srcGhostCnt"] > 0 and gs[1]["dstGhostCnt"] == 0
    assert stats[0][None] == stats[1][None] == (2, 1, 1, 2), stats


def test_golden_partition_with_a_3000_edge_row(da):
    """tests/golden/parts_hub3000_p2 (written by the reference's DataLoader): one row of 3 000 edges, walked by one lane group"""
    import partition_oracle as po
    dd = os.path.join(ROOT, "tests", "golden", "parts_hub3000_p2")
    bins = sorted(glob.glob(os.path.join(dd, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    gs = [po.parse_graph_bin(open(b, "rb").read()) for b in bins]
    parts = np.loadtxt(os.path.join(dd, "graph.bsnap.parts"), dtype=np.int64, ndmin=1)
    V = len(parts)
    src, dst = [], []
    for g in gs:                                            # the whole graph back from the partitions' in-edges
        N, l2g = g["localVtxCnt"], g["localToGlobal"].astype(np.int64)
        ids = np.concatenate([l2g, g["srcGhost"].astype(np.int64)])
        src.append(ids[g["rowIdx"]])
        dst.append(np.repeat(l2g, np.diff(g["colPtr"].astype(np.int64))))
    src, dst = np.concatenate(src), np.concatenate(dst)
    g_all = po.preprocess(src, dst, np.zeros(V, np.int64), 0, 1)
    assert int(g_all["localInEdgeCnt"]) == sum(int(g["localInEdgeCnt"]) for g in gs)
    assert max(np.diff(g["colPtr"].astype(np.int64)).max() for g in gs) >= 3000 or max(np.diff(g["rowPtr"].astype(np.int64)).max() for g in gs) >= 3000
    rng = np.random.default_rng(30)
    X = rng.uniform(-1, 1, (V, DIMS8[0])).astype(np.float32)
    labels = rng.integers(0, DIMS8[-1], V).astype(np.uint32)
    params = _params(rng, DIMS8, HEADS8)
    T, dW, stats = _partitioned(da, gs, parts, X, labels, params, DIMS8, HEADS8, {}, 1)
    _check(T, dW, _oracle(g_all, X, labels, params, HEADS8), "hub3000")


# ---- 5. peaked and flat attention ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 4.0])
def test_score_gradients_when_attention_is_flat_or_peaked(da, scale):
    """the bounds of test_gat_mh_sweep_score_gradients_when_attention_is_flat_or_peaked on the row-gather family (both layers take
    the row-wise destination side and the source side without dot products: differences of two sums of the size of t):
    |error| <= 5e-4 max|reference| + 32 eps max|t|, rows that touch an edge on LeakyReLU's kink apart"""
    import partition_oracle as po
    from helpers import rel_err
    dims, heads, V, E = [40, 128, 41], [8, 1], 600, 12000
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = []
    for l in range(2):
        zw = dims[l + 1]
        params.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                       (rng.standard_normal(zw) * scale).astype(np.float32), (rng.standard_normal(zw) * scale).astype(np.float32)])
    T, dW, stats = _single(da, g, X, labels, params, dims, heads, {})
    assert stats == (2, 0, 2, 2), stats
    fws, Hs, loss, dlogits, grads = _oracle(g, X, labels, params, heads)
    eps = 2.0 ** -23
    colptr, rowidx = np.asarray(g["colPtr"], np.int64), np.asarray(g["rowIdx"], np.int64)
    dst_of = np.repeat(np.arange(V), np.diff(colptr))
    for l in range(2):
        assert rel_err(T[(l, "o")], fws[l]["O"]) < RTOL, (scale, l, "o")
        assert np.abs(T[(l, "m")] - fws[l]["m"]).max() < 1e-4 * max(1.0, np.abs(fws[l]["m"]).max()), (scale, l, "m")     # the row maximum
        lse = np.log(T[(l, "den")].astype(np.float64)) + T[(l, "m")]
        assert np.abs(lse - (np.log(fws[l]["den"]) + fws[l]["m"])).max() < 1e-4, (scale, l, "log-sum-exp")
        tmax = np.abs(grads[l]["t"]).max()
        el, er = fws[l]["el"], fws[l]["er"]
        near = np.abs(el[rowidx] + er[dst_of]) < 2e-6
        skip_u, skip_v = np.zeros_like(el, dtype=bool), np.zeros_like(er, dtype=bool)
        np.logical_or.at(skip_u, rowidx, near)
        np.logical_or.at(skip_v, dst_of, near)
        selfnear = np.abs(el + er) < 2e-6
        skip_u |= selfnear
        skip_v |= selfnear
        assert skip_u.mean() < 0.05 and skip_v.mean() < 0.05, (scale, l, skip_u.mean(), skip_v.mean())
        for nm, key, skip in (("del", "d_el", skip_u), ("der", "d_er", skip_v)):
            got, ref = T[(l, nm)].astype(np.float64), grads[l][key]
            diff = np.abs(got[:, :ref.shape[1]] - ref)
            diff[skip] = 0.0
            err = diff.max()
            print(scale, l, nm, err, 5e-4 * np.abs(ref).max() + 32 * eps * tmax)
            assert err <= 5e-4 * np.abs(ref).max() + 32 * eps * tmax, (scale, l, nm, err, np.abs(ref).max(), tmax, int(skip.sum()))
        assert rel_err(T[(l, "dz")], grads[l]["dZ"]) < 5e-4, (scale, l, "dz")
        assert rel_err(dW[l]["w"], grads[l]["dW"]) < 5e-4, (scale, l, "dW")


# ---- 6. determinism ----------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(da):
    runs = [_hub_case(da, 2, [24, 64, 6], [4, 1], {"gatmh_sweep": 0, "gatmh_blocked": 0}, 0) for _ in range(2)]
    (Ta, dWa), (Tb, dWb) = runs[0][:2], runs[1][:2]
    for k in Ta:
        assert np.array_equal(Ta[k].view(np.uint32), Tb[k].view(np.uint32)), k
    for l in range(2):
        for nm in dWa[l]:
            assert np.array_equal(dWa[l][nm].view(np.uint32), dWb[l][nm].view(np.uint32)), (l, nm)


# ---- 7. the in-process transport: whole sweeps (gatmh_bwd_phase = 0), the family's own exchange call ---------------------------------------
def _local_run(da, dims, heads, epochs, merged, params):
    from local_ranks import run_local
    s, d, parts, rng = _hub_graph(2)
    parts = parts.astype(np.int32)
    V = len(parts)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    if params is None:
        params = _params(rng, dims, heads)
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.gatmh_row_gather(1)
        ctx.gatmh_bwd_merged_exchange(merged)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = (ctx.gatmh_row_gather_stats(), ctx.gatmh_bwd_merged_exchange_stats())
            close()
        ctx.close = closing
    pobjs = [da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, 2) for r in range(2)]
    dl = [(l, nm) for l in range(2) for nm in ("z", "el", "er", "o", "m", "den", "t", "del", "der", "dz")] + [(1, "logits"), (1, "grad"), (1, "h")]
    out = run_local(da, pobjs, parts, dims, da.GATMH, epochs, setup, {"gatmh_bwd_phase": 0}, downloads=dl,
                    pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r"))
    T = {}
    for k in dl:
        res = None
        for r, vw in enumerate(out["views"]):
            t = out["tensors"][r][k]
            if res is None:
                res = np.zeros((V, t.shape[1]), np.float32)
            res[vw["localToGlobal"]] = t
        T[k] = res
    return out, T, kept, (s, d, X, labels, params)


def test_in_process_transport_two_epochs_and_merged_exchange(da):
    """Two ranks over dory_comm_init_local, mode 1, whole sweeps: the family's phase 1, its call of the do / st exchange, its phase 2
    inside one dory_aggregate.  Epoch 1 against the oracle at the initial weights; epoch 2 against the oracle at the weights the
    ranks held after their first Adam step (the run is deterministic: the one-epoch run's final weights are the two-epoch run's
    weights during its second epoch).  Then the same two epochs with dory_gatmh_bwd_merged_exchange(1): the same bits."""
    import partition_oracle as po
    dims, heads = [24, 128, 6], [8, 1]
    one, T1, k1, (s, d, X, labels, params) = _local_run(da, dims, heads, 1, 0, None)
    g_all = po.preprocess(s, d, np.zeros(X.shape[0], np.int64), 0, 1)
    wg = lambda out: [{nm: out["wgrads"][0][l][nm] for nm in ("w", "a_l", "a_r")} for l in range(2)]     # (summed: identical on every rank)
    _check(T1, wg(one), _oracle(g_all, X, labels, params, heads), "epoch 1")
    W1 = [[one["weights"][0][l][nm].reshape(params[l][i].shape) for i, nm in enumerate(("w", "a_l", "a_r"))] for l in range(2)]
    two, T2, k2, _ = _local_run(da, dims, heads, 2, 0, params)
    _check(T2, wg(two), _oracle(g_all, X, labels, W1, heads), "epoch 2")
    for r in range(2):
        assert k2[r][0] == (4, 2, 2, 4) and k2[r][1] == (0, 0, 0, 0), (r, k2[r])
    mer, T3, k3, _ = _local_run(da, dims, heads, 2, 1, params)
    for k in T2:
        assert np.array_equal(T2[k].view(np.uint32), T3[k].view(np.uint32)), k
    for r in range(2):
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                assert np.array_equal(two["weights"][r][l][nm], mer["weights"][r][l][nm]), (r, l, nm)
                assert np.array_equal(two["wgrads"][r][l][nm], mer["wgrads"][r][l][nm]), (r, l, nm)
        assert k3[r][0] == (4, 2, 2, 4), (r, k3[r])
        assert k3[r][1][0] == 4 and k3[r][1][2] == 0 and k3[r][1][3] == 0, (r, k3[r])      # merged exchanges, none producer-packed


# ---- 8. contract -------------------------------------------------------------------------------------------------------------------------
def test_contract(da):
    import partition_oracle as po
    ctx = da.Context(0)
    ctx.configure(da.GCN, [8, 4, 3], 10)
    ctx.gatmh_row_gather(0)
    with pytest.raises(da.DoryError):
        ctx.gatmh_row_gather(1)                              # not a DORY_GATMH context
    ctx.close()
    dims, heads, V, E = [40, 128, 41], [8, 1], 300, 4000
    rng = np.random.default_rng(8)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = _params(rng, dims, heads)
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, V)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError):
            ctx.gatmh_row_gather(bad)
    ctx.close()
    # mode 0 on a graph the sweep forms take: the family does not run
    T, dW, stats = _single(da, g, X, labels, params, dims, heads, {"spmm_blk_nb": 8}, mode=0)
    assert stats == (0, 0, 0, 0), stats
    _check(T, dW, _oracle(g, X, labels, params, heads), "mode 0", true_max=False)     # (the sweep forms: m is their upper-bound shift)
    # bf16 rows: refused with the family forced, and the message says why
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, V)
    ctx.gatmh_heads(heads)
    ctx.set_option("spmm_blk_nb", 8)
    ctx.set_option("gatmh_bf16_gather", 1)
    ctx.gatmh_row_gather(1)
    ctx.graph_upload(g)
    ctx.preallocate()
    ctx.upload(0, "h", X)
    for l, (W, al, ar) in enumerate(params):
        ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
    ctx.apply_vertex(0, da.FORWARD)
    ctx.apply_edge(1, da.FORWARD)
    with pytest.raises(da.DoryError, match="dory_gatmh_row_gather = 1"):
        ctx.aggregate(1, da.FORWARD)
    assert ctx.gatmh_row_gather_stats() == (0, 0, 0, 0)
    ctx.close()
