"""dory_gatmh_row_gather_overlap (include/dorylus_hip.h): the multi-head GAT's row-gather kernels run the rows whose entries are all local
(row_interior_plan) in a launch of their own, before the wait for the exchange that fills the ghost rows, and the other rows after it
(csrc/gat_mh_rows.hip: the *_list_kernel forms).  Every row is computed whole by the body that computes it with the switch off, so every
comparison between the switch off and on is bit for bit.

  a. without an exchange in flight: one context per rank, gatmh_bwd_phase 1 / 2, the rows moved by halo_pack_tensor / halo_unpack_tensor;
  b. with the exchange in flight: whole epochs over the in-process transport, one thread per rank;
  c. nothing to split: one partition, a rank whose rows are all boundary rows, a rank without vertices;
  d. against the float64 oracle (oracle/gat_mh_oracle.py), the tolerances of tests/test_gpu_gatmh_row_gather.py;
  e. refusals on a live context."""
import numpy as np
import pytest

from test_gpu_gatmh_row_gather import _check, _hub_graph, _oracle, _params

pytestmark = pytest.mark.gpu
NAMES = ("z", "el", "er", "o", "m", "den", "t", "del", "der", "dz")
ZERO = dict(fwd_split=0, src_split=0, fwd_in_flight=0, src_in_flight=0, in_interior_rows=0, out_interior_rows=0, bwd_deferred=0)


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _block_graph(da, P, V=240, E=2600, blocks=None):
    """contiguous blocks of vertices, 85 % of the edges inside the destination's block: every rank has interior rows and boundary rows on
    both sides.  A boundary hub destination (7: 200 in-edges from anywhere), a boundary hub source (13), and an INTERIOR hub: 100 further
    edges into one vertex of block 0 whose sources are all in block 0.  Returns (s, d, parts, rng, interior hub's global id)."""
    import partition_oracle as po
    B = blocks or P
    rng = np.random.default_rng(17)
    parts = (np.arange(V) * B // V).astype(np.int64)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    intra = rng.random(E) < 0.85
    for e in np.where(intra)[0]:
        b = np.where(parts == parts[d[e]])[0]
        s[e] = b[rng.integers(0, len(b))]
    d[:200] = 7
    s[200:400] = 13
    hub = None
    if B > 1:
        g0 = po.preprocess(s, d, parts, 0, B)
        inter, _ = da.row_interior_plan(g0["colPtr"], g0["rowIdx"], g0["localVtxCnt"])
        hub = int(g0["localToGlobal"][[v for v in inter if g0["localToGlobal"][v] not in (7, 13)][0]])
        b0 = np.where(parts == 0)[0]
        s = np.concatenate([s, b0[np.random.default_rng(5).integers(0, len(b0), 100)]])
        d = np.concatenate([d, np.full(100, hub)])
    return s, d, parts, rng, hub


def _plans(da, gs):
    """[(in-interior, in-boundary, out-interior, out-boundary)] per rank, from the host plan"""
    return [da.row_interior_plan(g["colPtr"], g["rowIdx"], g["localVtxCnt"]) + da.row_interior_plan(g["rowPtr"], g["colIdx"], g["localVtxCnt"])
            for g in gs]


def _partitioned(da, gs, parts, X, labels, params, dims, heads, opts, setup, P=None):
    """the arrangement of tests/test_gpu_gatmh_row_gather.py::_partitioned: one epoch over one context per rank, the ghost rows moved by
    halo_pack_tensor / halo_unpack_tensor and a device copy, the backward in its phases 1 / 2; setup(ctx) sets the switches under test.
    Returns per rank: ({(layer, name): tensor}, weight gradients, the counters of the switch, of hub splitting, of the family)."""
    import torch
    from halo_plan_ref import halo_plan
    P, V, L = P or len(gs), len(parts), 2
    ctxs, plans = [], []
    for r, g in enumerate(gs):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V, r, P)
        ctx.gatmh_heads(heads)
        for k, v in opts.items():
            ctx.set_option(k, v)
        ctx.gatmh_row_gather(1)
        ctx.graph_upload(g)
        ctx.preallocate()
        setup(ctx)
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

    out = []
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
            T = {}
            if gs[r]["localVtxCnt"]:
                T = {(l, nm): c.download(l, nm) for l in range(L) for nm in NAMES}
                T.update({(1, nm): c.download(1, nm) for nm in ("logits", "grad", "h")})
            dW = [{nm: c.weight_grad_get(l, nm) for nm in ("w", "a_l", "a_r")} for l in range(L)]
            out.append((T, dW, c.gatmh_row_gather_overlap_stats(), c.gatmh_row_gather_hub_split_stats(), c.gatmh_row_gather_stats()))
    finally:
        for c in ctxs:
            c.close()
    return out


def _same(off, on, what):
    assert len(off) == len(on)
    for r, (a, b) in enumerate(zip(off, on)):
        assert a[0].keys() == b[0].keys(), (what, r)
        for k in a[0]:
            assert np.array_equal(_bits(a[0][k]), _bits(b[0][k])), (what, r, k, int((_bits(a[0][k]) != _bits(b[0][k])).sum()))
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                assert np.array_equal(_bits(a[1][l][nm]), _bits(b[1][l][nm])), (what, r, l, "d" + nm)


def _inputs(rng, V, dims, heads):
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    return X, labels, _params(rng, dims, heads)


def _case(da, P):
    """the block graph at P ranks: (edges, parts, rng, partitions, plans); asserts what the tests below rely on"""
    import partition_oracle as po
    s, d, parts, rng, hub = _block_graph(da, P)
    gs = [po.preprocess(s, d, parts, r, P) for r in range(P)]
    plans = _plans(da, gs)
    for r, (ii, ib, oi, ob) in enumerate(plans):
        print("P", P, "rank", r, "in", len(ii), "/", len(ib), "out", len(oi), "/", len(ob))
        assert len(ii) and len(ib) and len(oi) and len(ob), (P, r)
    l2g0 = gs[0]["localToGlobal"].astype(np.int64)
    h = int(np.flatnonzero(l2g0 == hub)[0])
    assert h in plans[0][0] and np.diff(gs[0]["colPtr"].astype(np.int64))[h] > 100         # the interior hub: interior, cut at 64
    b = int(np.flatnonzero(l2g0 == 7)[0])
    assert b in plans[0][1] and np.diff(gs[0]["colPtr"].astype(np.int64))[b] > 64          # the boundary hub
    return s, d, parts, rng, gs, plans


# (lane group, heads per float4) of the hidden layer; the last layer -- one head -- runs 8 lanes, one head per float4
SHAPES = [([24, 64, 6], [4, 1]),        # 16, 1
          ([24, 128, 6], [8, 1]),       # 32, 1
          ([24, 256, 6], [4, 1]),       # 64, 1
          ([24, 32, 6], [16, 1]),       # 8, 2
          ([24, 64, 6], [32, 1]),       # 16, 2
          ([24, 128, 6], [64, 1]),      # 32, 2
          ([16, 32, 5], [32, 1]),       # 8, 4
          ([24, 64, 6], [64, 1]),       # 16, 4
          ([24, 96, 6], [3, 1]),        # ld = 96: 32 lanes, the scores gathered from el / fg_el
          ([24, 160, 5], [5, 1]),       # ld = 160: 64 lanes, likewise
          ([24, 32, 8], [4, 2])]        # 8, 1 on both layers, two heads on the last
IDS = ["%s-%s" % ("x".join(map(str, d)), "x".join(map(str, h))) for d, h in SHAPES]


# ---- a. without an exchange in flight -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp32", "bf16", "hubs64"])
@pytest.mark.parametrize("dims,heads", SHAPES, ids=IDS)
@pytest.mark.parametrize("P", [2, 3])
def test_switch_off_against_on_nothing_in_flight(da, P, dims, heads, variant):
    s, d, parts, rng, gs, plans = _case(da, P)
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    opts = {"gatmh_bf16_gather": 2} if variant == "bf16" else {}

    def setup(on):
        def f(ctx):
            if variant == "bf16":
                ctx.gatmh_row_gather_bf16(1)
            if variant == "hubs64":
                ctx.gatmh_row_gather_hub_split(64)
            ctx.gatmh_row_gather_overlap(on)
        return f
    off = _partitioned(da, gs, parts, X, labels, params, dims, heads, opts, setup(0))
    on = _partitioned(da, gs, parts, X, labels, params, dims, heads, opts, setup(1))
    _same(off, on, (P, dims, heads, variant))
    for r in range(P):
        ii, ib, oi, ob = plans[r]
        assert off[r][2] == ZERO, (r, off[r][2])
        want = dict(ZERO, fwd_split=2, src_split=2, in_interior_rows=len(ii), out_interior_rows=len(oi))
        assert on[r][2] == want, (r, on[r][2], want)
        assert on[r][3] == off[r][3] and on[r][4] == off[r][4], (r, on[r][3:], off[r][3:])       # the same passes, the same hub plans
        if variant == "hubs64" and r == 0:              # (rank 0 owns the three hubs; both hub destinations are cut)
            hs = on[r][3]
            assert hs["fwd"] == 2 and hs["src"] == 2 and hs["in_hub_rows"] == 2 and hs["out_hub_rows"] == 1, (r, hs)
        if variant == "bf16":
            assert on[r][4][0] == 2 and on[r][4][3] == 2, (r, on[r][4])


# ---- b. with the exchange in flight ---------------------------------------------------------------------------------------------------
DIMS_B, HEADS_B, EPOCHS = [40, 128, 41], [8, 1], 2


def _epochs(da, Pn, on, merged, opts=None, bf16=False):
    """whole epochs over dory_comm_init_local, one thread per rank, mode 1; (run_local's result, {rank: counters before the context closes})"""
    from local_ranks import run_local
    s, d, parts, rng, hub = _block_graph(da, Pn)
    dims, heads, L = DIMS_B, HEADS_B, 2
    V = len(parts)
    X, labels, params = _inputs(rng, V, dims, heads)
    pobjs = [da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts.astype(np.int32), r, Pn) for r in range(Pn)]
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.gatmh_row_gather(1)
        ctx.gatmh_bwd_merged_exchange(merged)
        if bf16:
            ctx.gatmh_row_gather_bf16(1)
            ctx.halo_bf16_rows(1)
            ctx.gatmh_halo_bf16(1)
            ctx.halo_bf16_ghosts(1)
            ctx.gatmh_bf16_ghosts(1)
        ctx.gatmh_row_gather_overlap(on)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"ovl": ctx.gatmh_row_gather_overlap_stats(), "rows": ctx.gatmh_row_gather_stats(),
                           "plan": (da.row_interior_plan(g["colPtr"], g["rowIdx"], g["localVtxCnt"]),
                                    da.row_interior_plan(g["rowPtr"], g["colIdx"], g["localVtxCnt"]))}
            close()
        ctx.close = closing
    dl = [(l, nm) for l in range(L) for nm in NAMES + ("op", "dpos", "st", "do", "fg_z", "fg_el", "bg_do", "bg_st")] + [(L - 1, "logits"), (L - 1, "grad")]
    o = dict({"gatmh_bwd_phase": 0, "halo_overlap": 1}, **(opts or {}))
    if bf16:
        o["gatmh_bf16_gather"] = 2
    out = run_local(da, pobjs, parts.astype(np.int32), dims, da.GATMH, EPOCHS, setup, o, downloads=dl, pre=lambda c: c.gatmh_heads(heads),
                    wnames=("w", "a_l", "a_r"))
    return out, kept


def _same_run(a, b, what):
    for r in range(len(a["tensors"])):
        assert a["tensors"][r].keys() == b["tensors"][r].keys() and len(a["tensors"][r]) >= 30, (what, r)
        for k in a["tensors"][r]:
            assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


def _flight_counters(kon, koff, Pn, flight, deferred, what):
    L = 2
    for r in range(Pn):
        assert koff[r]["ovl"] == ZERO, (what, r, koff[r])
        (ii, ib), (oi, ob) = kon[r]["plan"]
        assert len(ii) and len(ib) and len(oi) and len(ob), (what, r)
        want = dict(fwd_split=L * EPOCHS, src_split=L * EPOCHS, fwd_in_flight=flight, src_in_flight=flight, in_interior_rows=len(ii),
                    out_interior_rows=len(oi), bwd_deferred=deferred)
        assert kon[r]["ovl"] == want, (what, r, kon[r]["ovl"], want)
        assert kon[r]["rows"] == koff[r]["rows"], (what, r)


@pytest.mark.parametrize("merged", [1, 0], ids=["merged", "two-exchanges"])
@pytest.mark.parametrize("Pn", [2, 3])
def test_epochs_with_the_exchange_in_flight(da, Pn, merged):
    """halo_overlap = 1: the forward's interior rows run beside the exchange of z, the source side's beside the backward's last exchange
    -- the merged one, or st's (do's, the first of two, is never deferred): one deferred backward exchange per layer and epoch either way"""
    off, koff = _epochs(da, Pn, 0, merged)
    on, kon = _epochs(da, Pn, 1, merged)
    _same_run(off, on, (Pn, merged))
    _flight_counters(kon, koff, Pn, 2 * EPOCHS, 2 * EPOCHS, (Pn, merged))


def test_epochs_in_flight_bf16_rows_wire_and_twins(da):
    off, koff = _epochs(da, 2, 0, 1, bf16=True)
    on, kon = _epochs(da, 2, 1, 1, bf16=True)
    _same_run(off, on, "bf16")
    _flight_counters(kon, koff, 2, 2 * EPOCHS, 2 * EPOCHS, "bf16")


def test_epochs_in_flight_halo_direct_recv(da):
    """the adjacency is renumbered, ghost ids stay >= N: the same lists; the merged exchange is not taken under such a plan (two exchanges)"""
    off, koff = _epochs(da, 2, 0, 1, {"halo_direct_recv": 1})
    on, kon = _epochs(da, 2, 1, 1, {"halo_direct_recv": 1})
    _same_run(off, on, "direct")
    _flight_counters(kon, koff, 2, 2 * EPOCHS, 2 * EPOCHS, "direct")


def test_epochs_without_halo_overlap_still_split(da):
    off, koff = _epochs(da, 2, 0, 1, {"halo_overlap": 0})
    on, kon = _epochs(da, 2, 1, 1, {"halo_overlap": 0})
    _same_run(off, on, "halo_overlap = 0")
    _flight_counters(kon, koff, 2, 0, 0, "halo_overlap = 0")
    ref, _ = _epochs(da, 2, 1, 1)                       # ... and the schedule does not change a bit either
    _same_run(ref, on, "halo_overlap 1 against 0")


# ---- c. nothing to split --------------------------------------------------------------------------------------------------------------
def _off_on(da, gs, parts, rng, dims, heads, P=None):
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    runs = [_partitioned(da, gs, parts, X, labels, params, dims, heads, {}, lambda ctx, on=on: ctx.gatmh_row_gather_overlap(on), P=P)
            for on in (0, 1)]
    _same(runs[0], runs[1], "nothing to split")
    return runs


def test_single_partition_has_nothing_to_split(da):
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 1)
    gs = [po.preprocess(s, d, parts, 0, 1)]
    off, on = _off_on(da, gs, parts, rng, [24, 128, 6], [8, 1])
    assert on[0][2] == dict(ZERO, in_interior_rows=on[0][2]["in_interior_rows"], out_interior_rows=on[0][2]["out_interior_rows"]), on[0][2]
    assert on[0][2]["fwd_split"] == 0 and on[0][2]["src_split"] == 0 and on[0][4][0] == 2


def test_ranks_whose_rows_are_all_boundary_rows(da):
    """scattered ownership, and every vertex with one in-edge and one out-edge across ranks"""
    import partition_oracle as po
    P = 4
    s, d, parts, rng = _hub_graph(P)
    V = len(parts)
    other = np.array([next(u for u in ((v + k) % V for k in range(1, V)) if parts[u] != parts[v]) for v in range(V)])
    s, d = np.concatenate([s, other, np.arange(V)]), np.concatenate([d, np.arange(V), other])
    gs = [po.preprocess(s, d, parts, r, P) for r in range(P)]
    for r, (ii, ib, oi, ob) in enumerate(_plans(da, gs)):
        assert len(ii) == 0 and len(oi) == 0 and len(ib) == len(ob) == gs[r]["localVtxCnt"] > 0, r
    off, on = _off_on(da, gs, parts, rng, [24, 128, 6], [8, 1])
    for r in range(P):
        assert on[r][2] == ZERO and on[r][4] == off[r][4] and on[r][4][0] == 2, (r, on[r][2], on[r][4])


def test_a_rank_without_vertices(da):
    """three ranks, the third owns nothing: its passes launch nothing, its counters stay 0; the other two split as ever"""
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 3, blocks=2)
    gs = [po.preprocess(s, d, parts, r, 3) for r in range(3)]
    assert gs[2]["localVtxCnt"] == 0
    off, on = _off_on(da, gs, parts, rng, [24, 128, 6], [8, 1], P=3)
    assert on[2][2] == ZERO and on[2][4] == (0, 0, 0, 0), on[2]
    for r in range(2):
        assert on[r][2]["fwd_split"] == 2 and on[r][2]["src_split"] == 2, (r, on[r][2])


# ---- d. against the float64 oracle ------------------------------------------------------------------------------------------------------
def test_switch_on_vs_oracle(da):
    import partition_oracle as po
    P, dims, heads = 3, [24, 128, 6], [8, 1]
    s, d, parts, rng, gs, plans = _case(da, P)
    V = len(parts)
    X, labels, params = _inputs(rng, V, dims, heads)
    on = _partitioned(da, gs, parts, X, labels, params, dims, heads, {}, lambda ctx: ctx.gatmh_row_gather_overlap(1))
    T = {}
    for r, g in enumerate(gs):
        assert on[r][2]["fwd_split"] == 2 and on[r][2]["src_split"] == 2, (r, on[r][2])
        for k, t in on[r][0].items():
            T.setdefault(k, np.zeros((V, t.shape[1]), np.float32))[g["localToGlobal"]] = t
    dW = [{nm: sum(on[r][1][l][nm] for r in range(P)) for nm in ("w", "a_l", "a_r")} for l in range(2)]
    g_all = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    _check(T, dW, _oracle(g_all, X, labels, params, heads), ("overlap", P))


# ---- e. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context(da):
    import partition_oracle as po
    c = da.Context(0)
    try:
        c.configure(da.GCN, [4, 16, 2], 100, 0, 2)
        with pytest.raises(da.DoryError, match="gatmh_row_gather_overlap.*DORY_GATMH"):
            c.gatmh_row_gather_overlap(1)
        c.gatmh_row_gather_overlap(0)
    finally:
        c.close()
    s, d, parts, rng, gs, plans = _case(da, 2)
    dims, heads = [24, 128, 6], [8, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    ctx = da.Context(0)
    try:
        ctx.configure(da.GATMH, dims, len(parts))        # (one node: an epoch graph records single partitions only; the rank's ghosts stay)
        ctx.gatmh_heads(heads)
        ctx.gatmh_row_gather(1)
        for bad in (2, -1):
            with pytest.raises(da.DoryError, match="gatmh_row_gather_overlap.*neither 0 nor 1"):
                ctx.gatmh_row_gather_overlap(bad)
        ctx.gatmh_row_gather_overlap(1)                  # before the graph: the first pass plans
        ctx.graph_upload(gs[0])
        ctx.preallocate()
        assert ctx.gatmh_row_gather_overlap_stats() == ZERO
        ctx.upload(0, "h", X[gs[0]["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_edge(1, da.FORWARD)
        # a recording whose first use would have to build the plan
        ctx.epoch_graph_begin()
        try:
            with pytest.raises(da.DoryError, match="run one eager epoch first"):
                ctx.aggregate(1, da.FORWARD)
            for on in (0, 1):
                with pytest.raises(da.DoryError, match="gatmh_row_gather_overlap: not while an epoch graph is being recorded"):
                    ctx.gatmh_row_gather_overlap(on)
        finally:
            ctx.epoch_graph_drop()
        assert ctx.gatmh_row_gather_overlap_stats() == ZERO
        ctx.aggregate(1, da.FORWARD)                     # eager: plans and splits
        st = ctx.gatmh_row_gather_overlap_stats()
        assert st == dict(ZERO, fwd_split=1, in_interior_rows=len(plans[0][0]), out_interior_rows=0), st
        ctx.gatmh_row_gather_overlap(0)
        ctx.gatmh_row_gather_overlap(1)                  # with a graph: both plans at once
        st = ctx.gatmh_row_gather_overlap_stats()
        assert st["in_interior_rows"] == len(plans[0][0]) and st["out_interior_rows"] == len(plans[0][2]), st
    finally:
        ctx.close()
