"""dory_gatmh_row_gather_hub_split (include/dorylus_hip.h; csrc/gat_mh_rows.hip): hub rows of the multi-head GAT's row-gather family cut
into chunks that run on lane groups of their own and are merged in chunk order.

The graph is tests/test_gpu_gatmh_row_gather.py::_hub_graph -- 240 vertices, a destination of 200 in-edges and a source of 200 out-edges,
scattered owners -- at chunk size 64: four chunks, a last chunk whose length is no multiple of four, the self edge in it.  Comparisons with
oracle/gat_mh_oracle.py (float64) use the tolerances of tests/test_gpu_gatmh_row_gather.py::_check; everything else is bit for bit.

  1. whole epochs against the oracle, one head shape per code path, two ranks and one forced partition;
  2. bits: a chunk size above every degree changes nothing; at 64 m keeps its bits on every row, o / op / den / dpos on every row
     that is not cut; two runs agree;
  3. the edges of the rule: degrees chunk - 1, chunk, chunk + 1; a hub whose sources are all ghosts; a hub on a rank without ghosts; a
     rank that owns nothing;
  4. peaked and flat attention;   5. bf16 rows (and ghost twins);   6. the golden partition with a row of 3 000 entries;
  7. the backward in its phases;   8. refusals;   9. the epoch graph."""
import glob
import os

import numpy as np
import pytest

import test_gpu_gatmh_row_gather as base
from test_gpu_gatmh_bf16_gather import make_gatmh, same_bits

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK = 64
NAMES = ("z", "el", "er", "o", "op", "m", "den", "dpos", "t", "del", "der", "st", "dz")
# one head shape per code path: one head per float4 on 16 / 32 / 64 lanes, two and four heads per float4, scores gathered (96 floats:
# 24 float4, no power of two), a single head
SHAPES = [([24, 64, 6], [4, 1]), ([24, 128, 6], [8, 1]), ([24, 256, 9], [32, 1]), ([24, 64, 6], [32, 1]), ([16, 32, 5], [32, 1]),
          ([24, 96, 6], [3, 1]), ([12, 100, 6], [1, 1])]
IDS = ["4x16", "8x16", "32x8", "32x2", "32x1", "3x32", "1x100"]


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


class HubDa:
    """the package as the helpers of the other test files see it, with contexts that have hub splitting set from birth and leave their
    counters behind (stats, in the order of creation) when they are closed"""

    def __init__(self, da, chunk):
        self._da, self.chunk, self.stats = da, chunk, []

    def __getattr__(self, k):
        return getattr(self._da, k)

    def Context(self, device=0):
        ctx = self._da.Context(device)
        ctx.gatmh_row_gather_hub_split(self.chunk)
        close, i = ctx.close, len(self.stats)
        self.stats.append(None)

        def closing():
            if ctx.h:
                self.stats[i] = ctx.gatmh_row_gather_hub_split_stats()
            close()
        ctx.close = closing
        return ctx


def _plan_counts(g, chunk):
    """(hub rows, chunks) of the in-edges and of the out-edges of a partition, from the definition"""
    out = []
    for key in ("colPtr", "rowPtr"):
        deg = np.diff(np.asarray(g[key], np.int64))
        hub = deg[deg > chunk]
        out += [int(hub.size), int(np.sum(-(-hub // chunk)))]
    return tuple(out)


def _check_stats(st, g, chunk, edge_passes=None):
    want = _plan_counts(g, chunk)
    got = (st["in_hub_rows"], st["in_chunks"], st["out_hub_rows"], st["out_chunks"])
    assert got == want, (got, want)
    assert st["fwd"] == (2 if want[0] else 0) and st["src"] == (2 if want[2] else 0), (st, want)
    if edge_passes is not None:
        assert st["dst_edge_pass"] == (edge_passes if want[0] else 0), (st, want, edge_passes)


# ---- 1. whole epochs against the oracle ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims,heads", SHAPES, ids=IDS)
def test_two_rank_epoch_vs_oracle(da, dims, heads):
    hda = HubDa(da, CHUNK)
    T, dW, stats, inp, gs = base._hub_case(hda, 2, dims, heads, {}, 1)
    base._check(T, dW, base._oracle(*inp, heads), ("hubs", 2, dims, heads))
    total = np.zeros(4, np.int64)
    for r, g in enumerate(gs):
        _check_stats(hda.stats[r], g, CHUNK, stats[r][None][base.EDGE])
        total += _plan_counts(g, CHUNK)
    assert total[0] >= 1 and total[1] >= 4 and total[2] >= 1 and total[3] >= 4, total      # hub rows and chunks on both adjacencies


@pytest.mark.parametrize("dims,heads", SHAPES, ids=IDS)
def test_forced_single_partition_epoch_vs_oracle(da, dims, heads):
    """gatmh_sweep = 0: every destination side is an edge pass, so the wide layer's edge pass is split too"""
    import partition_oracle as po
    s, d, parts, rng = base._hub_graph(1)
    V = len(parts)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = base._params(rng, dims, heads)
    hda = HubDa(da, CHUNK)
    T, dW, stats = base._single(hda, g, X, labels, params, dims, heads, {"gatmh_sweep": 0})
    base._check(T, dW, base._oracle(g, X, labels, params, heads), ("hubs", 1, dims, heads))
    assert stats == (2, 2, 0, 2), stats
    _check_stats(hda.stats[0], g, CHUNK, 2)
    assert _plan_counts(g, CHUNK) == (1, 4, 1, 4)


# ---- 2. bits ------------------------------------------------------------------------------------------------------------------------------
def _hub_inputs(dims, heads, seed=17):
    import partition_oracle as po
    s, d, parts, rng = base._hub_graph(1)
    V = len(parts)
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    return g, X, labels, base._params(rng, dims, heads)


def _engine(da, g, X, labels, params, dims, heads, opts, chunk, bf16=0):
    """one epoch inside the Engine on one forced partition: (tensors, weights and gradients after the Adam step, hub counters)"""
    ctx = make_gatmh(da, g, dims, heads, X.shape[0], X, labels, params, opts)
    try:
        ctx.gatmh_row_gather(1)
        if bf16:
            ctx.gatmh_row_gather_bf16(1)
            ctx.set_option("gatmh_bf16_gather", bf16)
        ctx.gatmh_row_gather_hub_split(chunk)
        ctx.adam_config(0.01)
        eng = da.NativeEngine(ctx)
        eng.run(1)
        T = {(l, nm): ctx.download(l, nm) for l in range(2) for nm in NAMES}
        T.update({k: ctx.download(*k) for k in ((1, "logits"), (1, "grad"), (1, "h"))})
        W = {(l, nm): ctx.weight_get(l, nm) for l in range(2) for nm in ("w", "a_l", "a_r")}
        W.update({(l, "d" + nm): ctx.weight_grad_get(l, nm) for l in range(2) for nm in ("w", "a_l", "a_r")})
        st = ctx.gatmh_row_gather_hub_split_stats()
        eng.close()
    finally:
        ctx.close()
    return T, W, st


@pytest.mark.parametrize("dims,heads,opts", [([24, 128, 6], [8, 1], {}), ([16, 32, 5], [32, 1], {"gatmh_sweep": 0})], ids=["8x16", "32x1"])
def test_bits_of_rows_that_are_not_cut(da, dims, heads, opts):
    g, X, labels, params = _hub_inputs(dims, heads)
    deg_in = np.diff(np.asarray(g["colPtr"], np.int64))
    assert deg_in.max() < 1024 and np.diff(np.asarray(g["rowPtr"], np.int64)).max() < 1024
    off = _engine(da, g, X, labels, params, dims, heads, opts, 0)
    big = _engine(da, g, X, labels, params, dims, heads, opts, 1024)
    # a chunk size above every degree: no hub row, the launches of the switched-off run, every bit of it
    assert big[2] == dict.fromkeys(da.Context.GATMH_HUB_SPLIT_STATS, 0), big[2]
    for k in off[0]:
        assert same_bits(off[0][k], big[0][k]), k
    for k in off[1]:
        assert same_bits(off[1][k], big[1][k]), k
    # chunk size 64: the maximum is exact -- m keeps its bits on every row; a row that is not cut keeps o, op, den, dpos
    on = _engine(da, g, X, labels, params, dims, heads, opts, CHUNK)
    assert on[2]["in_hub_rows"] == 1 and on[2]["in_chunks"] == 4 and on[2]["fwd"] == 2, on[2]
    whole = deg_in <= CHUNK
    assert (~whole).sum() == 1
    assert same_bits(off[0][(0, "m")], on[0][(0, "m")])
    for nm in ("o", "op", "den", "dpos"):
        assert same_bits(off[0][(0, nm)][whole], on[0][(0, nm)][whole]), nm
    cut = np.nonzero(~whole)[0][0]
    assert not same_bits(off[0][(0, "o")][cut], on[0][(0, "o")][cut]) or not same_bits(off[0][(0, "den")][cut], on[0][(0, "den")][cut])
    # same input, same bits
    again = _engine(da, g, X, labels, params, dims, heads, opts, CHUNK)
    for k in on[0]:
        assert same_bits(on[0][k], again[0][k]), k
    for k in on[1]:
        assert same_bits(on[1][k], again[1][k]), k


def test_two_ranks_two_runs_give_the_same_bits(da):
    runs = [base._hub_case(HubDa(da, CHUNK), 2, [24, 64, 6], [4, 1], {"gatmh_sweep": 0, "gatmh_blocked": 0}, 0) for _ in range(2)]
    (Ta, dWa), (Tb, dWb) = runs[0][:2], runs[1][:2]
    for k in Ta:
        assert same_bits(Ta[k], Tb[k]), k
    for l in range(2):
        for nm in dWa[l]:
            assert same_bits(dWa[l][nm], dWb[l][nm]), (l, nm)


# ---- 3. the edges of the rule -------------------------------------------------------------------------------------------------------------
def test_degrees_next_to_the_chunk_size(da):
    """destinations 1, 2, 3 with 63, 64, 65 in-edges, sources 4, 5, 6 with 63, 64, 65 out-edges: only the rows of 65 are cut, in two"""
    import partition_oracle as po
    V = 150
    rng = np.random.default_rng(5)
    s, d = list(rng.integers(10, V, 300)), list(rng.integers(10, V, 300))
    for i, n in enumerate((CHUNK - 1, CHUNK, CHUNK + 1)):
        s += list(rng.integers(10, V, n)); d += [1 + i] * n
        s += [4 + i] * n; d += list(rng.integers(10, V, n))
    g = po.preprocess(np.array(s), np.array(d), np.zeros(V, np.int64), 0, 1)
    assert list(np.diff(np.asarray(g["colPtr"], np.int64))[1:4]) == [63, 64, 65] and list(np.diff(np.asarray(g["rowPtr"], np.int64))[4:7]) == [63, 64, 65]
    assert _plan_counts(g, CHUNK) == (1, 2, 1, 2)
    X = rng.uniform(-1, 1, (V, base.DIMS8[0])).astype(np.float32)
    labels = rng.integers(0, base.DIMS8[-1], V).astype(np.uint32)
    params = base._params(rng, base.DIMS8, base.HEADS8)
    hda = HubDa(da, CHUNK)
    T, dW, stats = base._single(hda, g, X, labels, params, base.DIMS8, base.HEADS8, {"gatmh_sweep": 0})
    base._check(T, dW, base._oracle(g, X, labels, params, base.HEADS8), "63 / 64 / 65")
    _check_stats(hda.stats[0], g, CHUNK, 2)


def test_a_hub_whose_sources_are_all_ghosts(da):
    """rank 0 owns the hub destination 0 and the hub source 1; all their neighbours live on rank 1"""
    rng = np.random.default_rng(6)
    V = 160
    parts = (np.arange(V) >= 40).astype(np.int64)
    s, d = rng.integers(2, V, 600), rng.integers(2, V, 600)
    s = np.concatenate([s, rng.integers(40, V, 150), np.full(150, 1)])
    d = np.concatenate([d, np.full(150, 0), rng.integers(40, V, 150)])
    hda = HubDa(da, CHUNK)
    gs, stats = base._two_rank_case(hda, s, d, parts, 6)
    g0 = gs[0]
    N = int(g0["localVtxCnt"])
    assert np.all(np.asarray(g0["rowIdx"])[int(g0["colPtr"][0]):int(g0["colPtr"][1])] >= N)         # vertex 0: ghost sources only
    assert np.all(np.asarray(g0["colIdx"])[int(g0["rowPtr"][1]):int(g0["rowPtr"][2])] >= N)         # vertex 1: ghost destinations only
    assert _plan_counts(g0, CHUNK) == (1, 3, 1, 3)
    for r in range(2):
        _check_stats(hda.stats[r], gs[r], CHUNK, stats[r][None][base.EDGE])


def test_a_hub_on_a_rank_without_ghosts(da):
    """every cross edge runs from rank 0 to rank 1: rank 0 has no ghost sources (a null fg_z) and owns a hub destination, rank 1 has no
    ghost destinations (a null bg_do) and owns a hub source"""
    rng = np.random.default_rng(4)
    V, E = 120, 700
    parts = (np.arange(V) >= 60).astype(np.int64)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    back = (parts[s] == 1) & (parts[d] == 0)
    d[back] = rng.integers(60, V, int(back.sum()))
    s = np.concatenate([s, rng.integers(1, 60, 100), np.full(100, 61)])
    d = np.concatenate([d, np.full(100, 0), rng.integers(62, V, 100)])
    hda = HubDa(da, CHUNK)
    gs, stats = base._two_rank_case(hda, s, d, parts, 4)
    assert gs[0]["srcGhostCnt"] == 0 and gs[0]["dstGhostCnt"] > 0 and gs[1]["srcGhostCnt"] > 0 and gs[1]["dstGhostCnt"] == 0
    assert _plan_counts(gs[0], CHUNK)[0] == 1 and _plan_counts(gs[1], CHUNK)[2] == 1
    for r in range(2):
        _check_stats(hda.stats[r], gs[r], CHUNK, stats[r][None][base.EDGE])


def test_a_rank_that_owns_nothing(da):
    s, d, parts, rng = base._hub_graph(2)
    hda = HubDa(da, CHUNK)
    gs, stats = base._two_rank_case(hda, s, d, np.zeros(len(parts), np.int64), 3)
    assert gs[1]["localVtxCnt"] == 0
    _check_stats(hda.stats[0], gs[0], CHUNK, stats[0][None][base.EDGE])
    assert hda.stats[1] == dict.fromkeys(da.Context.GATMH_HUB_SPLIT_STATS, 0), hda.stats[1]
    assert hda.stats[0]["in_chunks"] == 4 and hda.stats[0]["out_chunks"] == 4


# ---- 4. peaked and flat attention ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1e-3, 4.0])
def test_score_gradients_when_attention_is_flat_or_peaked(da, scale):
    """the bounds of tests/test_gpu_gatmh_row_gather.py::test_score_gradients_when_attention_is_flat_or_peaked on the hub graph at chunk
    size 64: |error| <= 5e-4 max|reference| + 32 eps max|t|, rows that touch an edge on LeakyReLU's kink apart.  At scale 4 the chunks'
    maxima lie far apart: the merge must give no NaN or Inf"""
    from helpers import rel_err
    dims, heads = [40, 128, 41], [8, 1]
    g, X, labels, _ = _hub_inputs(dims, heads)
    V = X.shape[0]
    rng = np.random.default_rng(17)
    params = []
    for l in range(2):
        zw = dims[l + 1]
        params.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                       (rng.standard_normal(zw) * scale).astype(np.float32), (rng.standard_normal(zw) * scale).astype(np.float32)])
    hda = HubDa(da, CHUNK)
    T, dW, stats = base._single(hda, g, X, labels, params, dims, heads, {})
    assert stats == (2, 0, 2, 2), stats
    assert hda.stats[0]["fwd"] == 2 and hda.stats[0]["src"] == 2, hda.stats[0]
    for k, t in T.items():
        assert np.isfinite(t).all(), k
    fws, Hs, loss, dlogits, grads = base._oracle(g, X, labels, params, heads)
    eps = 2.0 ** -23
    colptr, rowidx = np.asarray(g["colPtr"], np.int64), np.asarray(g["rowIdx"], np.int64)
    dst_of = np.repeat(np.arange(V), np.diff(colptr))
    for l in range(2):
        assert rel_err(T[(l, "o")], fws[l]["O"]) < base.RTOL, (scale, l, "o")
        assert np.abs(T[(l, "m")] - fws[l]["m"]).max() < 1e-4 * max(1.0, np.abs(fws[l]["m"]).max()), (scale, l, "m")
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


# ---- 5. bf16 rows -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("dims,heads", [SHAPES[1], SHAPES[3], SHAPES[4], SHAPES[5], SHAPES[6]], ids=[IDS[1], IDS[3], IDS[4], IDS[5], IDS[6]])
def test_split_bf16_passes_equal_split_fp32_passes_on_rounded_rows(da, dims, heads, P):
    """tests/test_gpu_gatmh_row_gather_bf16.py's scheme with hub splitting on in both contexts: A gathers bf16 rows (gatmh_bf16_gather = 2),
    B gathers fp32 rows rounded on the host; every pass, stage by stage, bit for bit"""
    from test_gpu_gatmh_row_gather_bf16 import _hub_ranks
    hda = HubDa(da, CHUNK)
    R = _hub_ranks(hda, P, dims, heads, 2, opts={"gatmh_sweep": 0} if P == 1 else None)
    try:
        R.epoch()
        edge = sum(R.edge_pass(l) for l in range(2))
        hubs = 0
        for r in R.live:
            assert R.A[r].gatmh_row_gather_bf16_stats() == (2, edge, 2), (r, R.A[r].gatmh_row_gather_bf16_stats())
            for side in (R.A, R.B):
                st = side[r].gatmh_row_gather_hub_split_stats()
                _check_stats(st, R.gs[r], CHUNK, edge)
                hubs += st["in_chunks"] + st["out_chunks"]
        assert hubs >= 16, hubs
    finally:
        R.close()


def test_split_bf16_passes_with_ghost_twins(da):
    """dory_gatmh_bf16_ghosts on against off (tests/test_gpu_gatmh_bf16_ghosts.py::Stages), hub splitting on on both sides: the split bf16
    passes gather the ghost rows from the twins and give the same bits"""
    from test_gpu_gatmh_bf16_ghosts import Stages
    hda = HubDa(da, CHUNK)
    S = Stages(hda, [24, 128, 6], [8, 1], 2)
    try:
        S.epoch()
        for r in range(2):
            a, b = S.A[r].gatmh_row_gather_hub_split_stats(), S.B[r].gatmh_row_gather_hub_split_stats()
            assert a == b, (r, a, b)
            _check_stats(a, S.gs[r], CHUNK)
        assert sum(S.A[r].gatmh_row_gather_hub_split_stats()["in_chunks"] for r in range(2)) == 4
        assert S.A[0].gatmh_bf16_ghosts_stats()["twin_reads_rows"] > 0
    finally:
        S.close()


# ---- 6. the golden partition ------------------------------------------------------------------------------------------------------------------
def _golden():
    import partition_oracle as po
    dd = os.path.join(ROOT, "tests", "golden", "parts_hub3000_p2")
    bins = sorted(glob.glob(os.path.join(dd, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    gs = [po.parse_graph_bin(open(b, "rb").read()) for b in bins]
    parts = np.loadtxt(os.path.join(dd, "graph.bsnap.parts"), dtype=np.int64, ndmin=1)
    V = len(parts)
    src, dst = [], []
    for g in gs:                                            # the whole graph back from the partitions' in-edges
        l2g = g["localToGlobal"].astype(np.int64)
        ids = np.concatenate([l2g, g["srcGhost"].astype(np.int64)])
        src.append(ids[g["rowIdx"]])
        dst.append(np.repeat(l2g, np.diff(g["colPtr"].astype(np.int64))))
    g_all = po.preprocess(np.concatenate(src), np.concatenate(dst), np.zeros(V, np.int64), 0, 1)
    return bins, gs, parts, g_all


def test_golden_partition_with_a_3000_edge_row_at_chunk_512(da):
    hda = HubDa(da, 512)
    base.test_golden_partition_with_a_3000_edge_row(hda)          # (two ranks, mode 1, against the oracle)
    bins, gs, parts, g_all = _golden()
    chunks = 0
    for r, g in enumerate(gs):
        _check_stats(hda.stats[r], g, 512)
        chunks += hda.stats[r]["in_chunks"] + hda.stats[r]["out_chunks"]
    assert chunks >= 6, [hda.stats[r] for r in range(2)]


def test_golden_partition_over_the_in_process_transport_with_the_merged_exchange(da):
    from local_ranks import run_local
    bins, gs, parts, g_all = _golden()
    dims, heads = base.DIMS8, base.HEADS8
    V = len(parts)
    rng = np.random.default_rng(30)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = base._params(rng, dims, heads)
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.gatmh_row_gather(1)
        ctx.gatmh_bwd_merged_exchange(1)
        ctx.gatmh_row_gather_hub_split(512)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = (ctx.gatmh_row_gather_hub_split_stats(), ctx.gatmh_bwd_merged_exchange_stats())
            close()
        ctx.close = closing
    pobjs = [da.Partition.load(b) for b in bins]
    dl = [(l, nm) for l in range(2) for nm in ("z", "el", "er", "o", "m", "den", "t", "del", "der", "dz")] + [(1, "logits"), (1, "grad"), (1, "h")]
    out = run_local(da, pobjs, parts.astype(np.int32), dims, da.GATMH, 1, setup, {"gatmh_bwd_phase": 0}, downloads=dl,
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
    dW = [{nm: out["wgrads"][0][l][nm] for nm in ("w", "a_l", "a_r")} for l in range(2)]
    base._check(T, dW, base._oracle(g_all, X, labels, params, heads), "hub3000, in-process, merged")
    for r, g in enumerate(gs):
        _check_stats(kept[r][0], g, 512)
        assert kept[r][1][0] == 2, (r, kept[r])                     # both layers' do / st went as one merged exchange
    assert sum(kept[r][0]["in_chunks"] + kept[r][0]["out_chunks"] for r in range(2)) >= 6


# ---- 7. the backward in its phases ------------------------------------------------------------------------------------------------------------
def test_backward_phases_1_then_2_give_the_whole_pass_bits(da):
    dims, heads = [24, 128, 6], [8, 1]
    g, X, labels, params = _hub_inputs(dims, heads)
    got = []
    for phases in ((0,), (1, 2)):
        ctx = make_gatmh(da, g, dims, heads, X.shape[0], X, labels, params, {"gatmh_sweep": 0})
        try:
            ctx.gatmh_row_gather(1)
            ctx.gatmh_row_gather_hub_split(CHUNK)
            for l in range(2):
                ctx.apply_vertex(l, da.FORWARD)
                ctx.apply_edge(l + 1, da.FORWARD)
                ctx.aggregate(l + 1, da.FORWARD)
            ctx.predict_gat(2)
            for l in (1, 0):
                for ph in phases:
                    ctx.set_option("gatmh_bwd_phase", ph)
                    ctx.aggregate(l + 1, da.BACKWARD)
                ctx.apply_vertex(l, da.BACKWARD)
            st = ctx.gatmh_row_gather_hub_split_stats()
            assert (st["fwd"], st["dst_edge_pass"], st["src"]) == (2, 2, 2), st
            out = {(l, nm): ctx.download(l, nm) for l in range(2) for nm in NAMES}
            out.update({(l, "d" + nm): ctx.weight_grad_get(l, nm) for l in range(2) for nm in ("w", "a_l", "a_r")})
            got.append(out)
        finally:
            ctx.close()
    for k in got[0]:
        assert same_bits(got[0][k], got[1][k]), k


# ---- 8. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(da):
    for gnn in (da.GCN, da.GAT):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        ctx.gatmh_row_gather_hub_split(0)
        for v in (64, 4096):
            with pytest.raises(da.DoryError, match="DORY_GATMH"):
                ctx.gatmh_row_gather_hub_split(v)
        ctx.close()
    dims, heads = [24, 64, 6], [4, 1]
    g, X, labels, params = _hub_inputs(dims, heads)
    ctx = make_gatmh(da, g, dims, heads, X.shape[0], X, labels, params, {})
    try:
        for bad in (1, 63, 65, 100, (1 << 20) + 64, 1 << 21):
            with pytest.raises(da.DoryError, match="multiple of 64"):
                ctx.gatmh_row_gather_hub_split(bad)
        assert ctx.gatmh_row_gather_hub_split_stats() == dict.fromkeys(da.Context.GATMH_HUB_SPLIT_STATS, 0)
        for ok in (64, 1 << 20, 128):                                # set with a graph there: the plans are built at once
            ctx.gatmh_row_gather_hub_split(ok)
        st = ctx.gatmh_row_gather_hub_split_stats()
        assert (st["in_hub_rows"], st["in_chunks"], st["out_hub_rows"], st["out_chunks"]) == _plan_counts(g, 128), st
        ctx.epoch_graph_begin()
        for v in (0, 64):
            with pytest.raises(da.DoryError, match="recorded"):
                ctx.gatmh_row_gather_hub_split(v)
        ctx.epoch_graph_drop()
        ctx.gatmh_row_gather_hub_split(0)
        assert ctx.gatmh_row_gather_hub_split_stats() == dict.fromkeys(da.Context.GATMH_HUB_SPLIT_STATS, 0)
        # a new upload drops the plans; the first pass that needs them builds them again
        ctx.gatmh_row_gather_hub_split(CHUNK)
        ctx.graph_upload(g)
        assert ctx.gatmh_row_gather_hub_split_stats()["in_chunks"] == 0
        ctx.gatmh_row_gather(1)
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_edge(1, da.FORWARD)
        ctx.aggregate(1, da.FORWARD)
        st = ctx.gatmh_row_gather_hub_split_stats()
        assert st["fwd"] == 1 and st["in_chunks"] == 4 and st["out_chunks"] == 0, st
    finally:
        ctx.close()


# ---- 9. the epoch graph -------------------------------------------------------------------------------------------------------------------------
def test_replayed_epochs_are_bit_identical_to_eager(da):
    """one partition, mode 1, chunk size 64: the first (eager) epoch builds the plans and sizes the scratch, the recording finds both; five
    epochs replayed equal five eager ones, and replays do not move the counters"""
    dims, heads = [24, 64, 6], [4, 1]
    g, X, labels, params = _hub_inputs(dims, heads)
    states = []
    for graph in (0, 1):
        ctx = make_gatmh(da, g, dims, heads, X.shape[0], X, labels, params, {"gatmh_sweep": 0})
        try:
            ctx.gatmh_row_gather(1)
            ctx.gatmh_row_gather_hub_split(CHUNK)
            ctx.adam_config(0.01)
            ctx.set_option("epoch_graph", graph)
            eng = da.NativeEngine(ctx)
            eng.run(3)
            eng.run(2)
            st = ctx.gatmh_row_gather_hub_split_stats()
            if graph:                               # one eager epoch and one recording
                assert ctx.get_option("epoch_graph_recorded") == 1
                assert (st["fwd"], st["dst_edge_pass"], st["src"]) == (4, 4, 4), st
            else:
                assert (st["fwd"], st["dst_edge_pass"], st["src"]) == (10, 10, 10), st
            out = {(l, nm): ctx.download(l, nm) for l in range(2) for nm in NAMES}
            for l in range(2):
                for nm in ("w", "a_l", "a_r"):
                    out[(nm, l)] = ctx.weight_get(l, nm)
                    out[("d" + nm, l)] = ctx.weight_grad_get(l, nm)
            states.append(out)
            eng.close()
        finally:
            ctx.close()
    for k in states[0]:
        assert same_bits(states[0][k], states[1][k]), k
