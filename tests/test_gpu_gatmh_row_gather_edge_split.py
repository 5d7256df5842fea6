"""dory_gatmh_row_gather_edge_split (include/dorylus_hip.h): the multi-head GAT's row-gather kernels walk every row's local entries and
its self edge before its ghost entries, over a local-first copy of the ids (row_edge_split_plan), and carry the row's state across the
wait for the exchange (csrc/gat_mh_rows.hip: the *_carry_kernel forms).  Value 1 runs one launch where nothing is in flight and two
around an exchange in flight, value 2 always two.

What is held bit for bit: one launch against two launches, in every tensor, weight and weight gradient; m of the first layer against
value 0 (a maximum does not depend on the order of the entries; the second layer's inputs already differ in their last bits); two runs.
Everything else changes association against value 0 and is held to the float64 oracle (oracle/gat_mh_oracle.py) with the tolerances of
tests/test_gpu_gatmh_row_gather.py::_check.

A bf16 pass equals the fp32 pass on rows rounded beforehand, bit for bit, with the switch on in both.

  1. range boundaries at every loop edge (a planted graph);      6. hub fallback;
  2. one shape per instantiation;                                7. the wide bf16 switch is not taken;
  3. whole epochs with the exchange in flight;                   8. the epoch graph;
  4. backward phases 1 / 2 against phase 0;                      9. two runs;
  5. nothing to split;                                          10. refusals on a live context."""
import numpy as np
import pytest

from test_gpu_gatmh_row_gather import _check, _oracle, _params
from test_gpu_gatmh_row_gather_overlap import IDS, NAMES, SHAPES, _bits, _block_graph, _inputs, _partitioned, _same, _same_run

pytestmark = pytest.mark.gpu
ZERO = dict(fwd_split=0, src_split=0, fwd_in_flight=0, src_in_flight=0, in_local_entries=0, out_local_entries=0, hub_fallbacks=0,
            wide_not_taken=0)
COUNTS = (0, 1, 3, 4, 5, 7, 8, 9, 15, 16, 17)          # 0, 1, 3, 4, 5 and GROUP - 1, GROUP, GROUP + 1 for lane groups of 8 and 16


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def _run(da, gs, parts, X, labels, params, dims, heads, value, opts=None, more=None, P=None):
    """tests/test_gpu_gatmh_row_gather_overlap.py::_partitioned with this switch at `value` (and more(ctx) before it); returns its result
    and, per rank, the counters of this switch read before the context closes"""
    kept = []

    def setup(ctx):
        if more:
            more(ctx)
        ctx.gatmh_row_gather_edge_split(value)
        close, r = ctx.close, len(kept)
        kept.append(None)

        def closing():
            if ctx.h:
                kept[r] = ctx.gatmh_row_gather_edge_split_stats()
            close()
        ctx.close = closing
    out = _partitioned(da, gs, parts, X, labels, params, dims, heads, opts or {}, setup, P=P)
    return out, kept


def _local_entries(da, g):
    N = g["localVtxCnt"]
    return tuple(int((mid - np.asarray(g[pk], np.uint64)[:-1]).sum())
                 for pk, mid in (("colPtr", da.row_edge_split_plan(g["colPtr"], g["rowIdx"], N)[1]),
                                 ("rowPtr", da.row_edge_split_plan(g["rowPtr"], g["colIdx"], N)[1])))


def _global(gs, out, V):
    """(tensors in global row order, weight gradients summed over the ranks) of a _partitioned result"""
    T = {}
    for r, g in enumerate(gs):
        for k, t in out[r][0].items():
            T.setdefault(k, np.zeros((V, t.shape[1]), np.float32))[g["localToGlobal"]] = t
    dW = [{nm: sum(out[r][1][l][nm] for r in range(len(gs))) for nm in ("w", "a_l", "a_r")} for l in range(2)]
    return T, dW


def _vs_oracle(gs, out, s, d, X, labels, params, heads, what):
    import partition_oracle as po
    V = X.shape[0]
    T, dW = _global(gs, out, V)
    _check(T, dW, _oracle(po.preprocess(s, d, np.zeros(V, np.int64), 0, 1), X, labels, params, heads), what)


def _m_of_the_first_layer(a, b, what):
    for r in range(len(a)):
        if (0, "m") in a[r][0]:
            assert np.array_equal(_bits(a[r][0][(0, "m")]), _bits(b[r][0][(0, "m")])), (what, r)


# ---- 1. range boundaries at every loop edge -------------------------------------------------------------------------------------------
def _planted():
    """240 vertices, two ranks of 120.  Rank 0's vertices 0..10 are destinations with (local, ghost) source counts that run through COUNTS
    on both sides, 40..50 sources with such destination counts; 12 has no edge at all; the rest is a random graph that touches none of
    them as the counted end."""
    V = 240
    rng = np.random.default_rng(29)
    parts = (np.arange(V) >= 120).astype(np.int64)
    pairs = [(a, COUNTS[(i + 3) % len(COUNTS)]) for i, a in enumerate(COUNTS)]
    s, d = [], []
    for i, (a, b) in enumerate(pairs):
        src = np.concatenate([80 + rng.permutation(40)[:a], 120 + rng.permutation(120)[:b]])
        s += list(rng.permutation(src)); d += [i] * (a + b)                      # in-edges of vertex i, local and ghost sources mixed
        dst = np.concatenate([60 + rng.permutation(20)[:a], 120 + rng.permutation(120)[:b]])
        s += [40 + i] * (a + b); d += list(rng.permutation(dst))                 # out-edges of vertex 40 + i
    bs, bd = 80 + rng.integers(0, 160, 1500), 60 + rng.integers(0, 180, 1500)
    keep = bs != bd
    s, d = np.concatenate([np.array(s, np.int64), bs[keep]]), np.concatenate([np.array(d, np.int64), bd[keep]])
    return s, d, parts, rng, pairs


@pytest.mark.parametrize("dims,heads", [([24, 32, 6], [4, 1]), ([24, 64, 6], [4, 1])], ids=["group8", "group16"])
def test_range_boundaries_at_every_loop_edge(da, dims, heads):
    import partition_oracle as po
    s, d, parts, rng, pairs = _planted()
    gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
    g, N = gs[0], gs[0]["localVtxCnt"]
    for pk, ik in (("colPtr", "rowIdx"), ("rowPtr", "colIdx")):
        ptr = np.asarray(g[pk], np.int64)
        _, mid = da.row_edge_split_plan(g[pk], g[ik], N)
        loc, gho = mid.astype(np.int64) - ptr[:-1], ptr[1:] - mid.astype(np.int64)
        assert set(COUNTS) <= set(loc.tolist()) and set(COUNTS) <= set(gho.tolist()), (pk, sorted(set(loc)), sorted(set(gho)))
        assert set(pairs) <= set(zip(loc.tolist(), gho.tolist())), pk
        assert np.any((loc == 0) & (gho == 0))               # a row with no entries at all
        assert np.any((loc == 0) & (gho > 0))                # a row whose only local entry is the self edge
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    one, k1 = _run(da, gs, parts, X, labels, params, dims, heads, 1)
    two, k2 = _run(da, gs, parts, X, labels, params, dims, heads, 2)
    _same(one, two, ("planted", dims))
    for r in range(2):
        li, lo = _local_entries(da, gs[r])
        want = dict(ZERO, fwd_split=2, src_split=2, in_local_entries=li, out_local_entries=lo)
        assert k1[r] == want and k2[r] == want, (r, k1[r], k2[r], want)
    _vs_oracle(gs, one, s, d, X, labels, params, heads, ("planted", dims))


# ---- 2. one shape per instantiation -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["fp32", "bf16"])
@pytest.mark.parametrize("dims,heads", SHAPES, ids=IDS)
@pytest.mark.parametrize("P", [2, 3])
def test_one_launch_against_two_per_instantiation(da, P, dims, heads, variant):
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, P)
    gs = [po.preprocess(s, d, parts, r, P) for r in range(P)]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    opts = {"gatmh_bf16_gather": 2} if variant == "bf16" else {}
    more = (lambda ctx: ctx.gatmh_row_gather_bf16(1)) if variant == "bf16" else None
    runs = [_run(da, gs, parts, X, labels, params, dims, heads, v, opts, more) for v in (0, 1, 2)]
    (off, k0), (one, k1), (two, k2) = runs
    _same(one, two, (P, dims, heads, variant))
    _m_of_the_first_layer(off, one, (P, dims, heads, variant))
    for r in range(P):
        assert k0[r] == ZERO, (r, k0[r])
        assert k1[r] == k2[r] and k1[r]["fwd_split"] == 2 and k1[r]["src_split"] == 2 and k1[r]["fwd_in_flight"] == 0, (r, k1[r], k2[r])
        assert one[r][4] == off[r][4], (r, one[r][4], off[r][4])                 # the family's passes: the same
    if variant == "fp32":      # (bf16 rows: rounding a row costs 2^-9, past the oracle's tolerances whatever the kernel -- they are held to
        _vs_oracle(gs, one, s, d, X, labels, params, heads, (P, dims, heads))    #  the fp32 passes on rounded rows, bit for bit, below)


@pytest.mark.parametrize("value", [1, 2])
@pytest.mark.parametrize("dims,heads", [([24, 64, 6], [4, 1]), ([24, 128, 6], [8, 1]), ([24, 64, 6], [32, 1]), ([16, 32, 5], [32, 1]),
                                        ([24, 96, 6], [3, 1])])
def test_bf16_carry_passes_equal_fp32_carry_passes_on_rounded_rows(da, dims, heads, value):
    """the family's standing rule, with the switch on in both contexts: tests/test_gpu_gatmh_row_gather_bf16.py's scheme (context A
    gathers bf16 rows, context B fp32 rows rounded on the host), every stage bit for bit"""
    from test_gpu_gatmh_row_gather_bf16 import _hub_ranks
    R = _hub_ranks(da, 2, dims, heads, 2)
    try:
        for c in R.all():
            c.gatmh_row_gather_edge_split(value)
        R.epoch()
        for r in R.live:
            for c in (R.A[r], R.B[r]):
                st = c.gatmh_row_gather_edge_split_stats()
                assert st["fwd_split"] == 2 and st["src_split"] == 2, (r, st)
    finally:
        R.close()


# ---- 3. whole epochs with the exchange in flight ------------------------------------------------------------------------------------------
DIMS_B, HEADS_B, EPOCHS = [40, 128, 41], [8, 1], 2


def _epochs(da, Pn, value, merged, opts=None, bf16=False, epochs=EPOCHS):
    """whole epochs over dory_comm_init_local, one thread per rank, mode 1; (run_local's result, {rank: counters before the context closes})"""
    from local_ranks import run_local
    s, d, parts, rng, hub = _block_graph(da, Pn)
    dims, heads, L = DIMS_B, HEADS_B, 2
    X, labels, params = _inputs(rng, len(parts), dims, heads)
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
        ctx.gatmh_row_gather_edge_split(value)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"es": ctx.gatmh_row_gather_edge_split_stats(), "rows": ctx.gatmh_row_gather_stats(),
                           "ovl": ctx.gatmh_row_gather_overlap_stats()}
            close()
        ctx.close = closing
    dl = [(l, nm) for l in range(L) for nm in NAMES + ("op", "dpos", "st", "do", "fg_z", "fg_el", "bg_do", "bg_st")] + [(L - 1, "logits"), (L - 1, "grad")]
    o = dict({"gatmh_bwd_phase": 0, "halo_overlap": 1}, **(opts or {}))
    if bf16:
        o["gatmh_bf16_gather"] = 2
    out = run_local(da, pobjs, parts.astype(np.int32), dims, da.GATMH, epochs, setup, o, downloads=dl, pre=lambda c: c.gatmh_heads(heads),
                    wnames=("w", "a_l", "a_r"))
    return out, kept


def _in_flight_against_not(da, Pn, merged, what, opts=None, bf16=False):
    """value 1 under halo_overlap = 1 (two launches around the exchange in flight) against halo_overlap = 0 (one launch) against value 2"""
    fl, kfl = _epochs(da, Pn, 1, merged, opts, bf16)
    no, kno = _epochs(da, Pn, 1, merged, dict(opts or {}, halo_overlap=0), bf16)
    _same_run(no, fl, what)
    for r in range(Pn):
        a, b = kfl[r]["es"], kno[r]["es"]
        assert a["fwd_split"] == b["fwd_split"] == 2 * EPOCHS and a["src_split"] == b["src_split"] == 2 * EPOCHS, (what, r, a, b)
        assert a["fwd_in_flight"] == 2 * EPOCHS and a["src_in_flight"] == 2 * EPOCHS, (what, r, a)          # every layer, every epoch
        assert b["fwd_in_flight"] == 0 and b["src_in_flight"] == 0, (what, r, b)
        assert a["hub_fallbacks"] == 0 and kfl[r]["rows"] == kno[r]["rows"], (what, r)
        assert kfl[r]["ovl"]["bwd_deferred"] == 2 * EPOCHS and kno[r]["ovl"]["bwd_deferred"] == 0, (what, r, kfl[r]["ovl"])
    return fl


@pytest.mark.parametrize("merged", [1, 0], ids=["merged", "two-exchanges"])
@pytest.mark.parametrize("Pn", [2, 3])
def test_epochs_with_the_exchange_in_flight(da, Pn, merged):
    fl = _in_flight_against_not(da, Pn, merged, (Pn, merged))
    two, _ = _epochs(da, Pn, 2, merged)
    _same_run(two, fl, (Pn, merged, "value 2"))


def test_epochs_in_flight_bf16_rows_wire_and_twins(da):
    _in_flight_against_not(da, 2, 1, "bf16", bf16=True)


def test_epochs_in_flight_halo_direct_recv(da):
    """the adjacency is uploaded renumbered: the copy is built from those ids"""
    _in_flight_against_not(da, 2, 1, "direct", {"halo_direct_recv": 1})


# ---- 4. backward phases ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("value", [1, 2])
def test_backward_phases_1_and_2_against_phase_0(da, value):
    """one epoch: the rows moved by halo_pack_tensor / halo_unpack_tensor between gatmh_bwd_phase 1 and 2, against the whole backward
    (phase 0) over the in-process transport"""
    import partition_oracle as po
    P = 2
    s, d, parts, rng, _ = _block_graph(da, P)
    gs = [po.preprocess(s, d, parts, r, P) for r in range(P)]
    X, labels, params = _inputs(rng, len(parts), DIMS_B, HEADS_B)
    ph12, _ = _run(da, gs, parts, X, labels, params, DIMS_B, HEADS_B, value)
    ph0, _ = _epochs(da, P, value, 0, epochs=1)
    for r in range(P):
        for l in range(2):
            for nm in NAMES:
                assert np.array_equal(_bits(ph12[r][0][(l, nm)]), _bits(ph0["tensors"][r][(l, nm)])), (value, r, l, nm)
            for nm in ("w", "a_l", "a_r"):       # (the engine sums the weight gradients over the two ranks: one fp32 addition, either order)
                both = np.asarray(ph12[0][1][l][nm], np.float32) + np.asarray(ph12[1][1][l][nm], np.float32)
                assert np.array_equal(_bits(both), _bits(ph0["wgrads"][r][l][nm])), (value, r, l, "d" + nm)


# ---- 5. nothing to split ------------------------------------------------------------------------------------------------------------------
def test_single_partition_has_nothing_to_split(da):
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 1)
    gs = [po.preprocess(s, d, parts, 0, 1)]
    dims, heads = [24, 128, 6], [8, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    off, k0 = _run(da, gs, parts, X, labels, params, dims, heads, 0)
    for v in (1, 2):
        on, k = _run(da, gs, parts, X, labels, params, dims, heads, v)
        _same(off, on, ("one partition", v))
        assert k[0] == ZERO and on[0][4] == off[0][4] and on[0][4][0] == 2, (v, k[0], on[0][4])


def test_a_rank_without_vertices(da):
    """three ranks, the third owns nothing: its passes launch nothing, its counters stay 0; the other two split"""
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 3, blocks=2)
    gs = [po.preprocess(s, d, parts, r, 3) for r in range(3)]
    assert gs[2]["localVtxCnt"] == 0
    dims, heads = [24, 128, 6], [8, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    off, _ = _run(da, gs, parts, X, labels, params, dims, heads, 0, P=3)
    one, k1 = _run(da, gs, parts, X, labels, params, dims, heads, 1, P=3)
    two, k2 = _run(da, gs, parts, X, labels, params, dims, heads, 2, P=3)
    _same(one, two, "empty rank")
    assert k1[2] == ZERO and k2[2] == ZERO and one[2][4] == off[2][4] == (0, 0, 0, 0), (k1[2], one[2][4])
    for r in range(2):
        assert k1[r]["fwd_split"] == 2 and k1[r]["src_split"] == 2, (r, k1[r])


def test_ghosts_on_one_side_only(da):
    """every edge between the ranks runs from rank 1 to rank 0: rank 0 has ghost sources and no ghost destination, rank 1 the reverse --
    each splits the one pass that has something to split, and the other pass launches what value 0 launches"""
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 2)
    back = (parts[s] == 0) & (parts[d] == 1)
    s, d = s[~back], d[~back]
    gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
    assert gs[0]["srcGhostCnt"] and not gs[0]["dstGhostCnt"] and gs[1]["dstGhostCnt"] and not gs[1]["srcGhostCnt"]
    dims, heads = [24, 128, 6], [8, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    off, _ = _run(da, gs, parts, X, labels, params, dims, heads, 0)
    one, k1 = _run(da, gs, parts, X, labels, params, dims, heads, 1)
    two, k2 = _run(da, gs, parts, X, labels, params, dims, heads, 2)
    _same(one, two, "one side")
    assert (k1[0]["fwd_split"], k1[0]["src_split"]) == (2, 0) and (k1[1]["fwd_split"], k1[1]["src_split"]) == (0, 2), k1
    assert k1 == k2 and k1[0]["out_local_entries"] == 0 and k1[1]["in_local_entries"] == 0, (k1, k2)
    for nm in ("o", "m", "den"):       # rank 1's first forward reads no ghost row and nothing an edge-split pass wrote: value 0's launch, value 0's bits
        assert np.array_equal(_bits(one[1][0][(0, nm)]), _bits(off[1][0][(0, nm)])), nm
    _vs_oracle(gs, one, s, d, X, labels, params, heads, "one side")


# ---- 6. hub fallback ----------------------------------------------------------------------------------------------------------------------
def test_hub_rows_fall_back_to_the_chunk_plan(da):
    """chunk size 64 and hub rows in both adjacencies of both ranks: no pass is taken, every pass is counted, every bit is value 0's"""
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 2)
    r2 = np.random.default_rng(3)
    s = np.concatenate([s, r2.integers(0, 240, 100), np.full(100, 210)])         # rank 1: a hub destination (200) and a hub source (210)
    d = np.concatenate([d, np.full(100, 200), r2.integers(0, 240, 100)])
    gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
    dims, heads = [24, 128, 6], [8, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    hub = lambda ctx: ctx.gatmh_row_gather_hub_split(64)
    off, k0 = _run(da, gs, parts, X, labels, params, dims, heads, 0, more=hub)
    on, k1 = _run(da, gs, parts, X, labels, params, dims, heads, 1, more=hub)
    _same(off, on, "hub fallback")
    for r in range(2):
        hs = on[r][3]
        assert hs["in_hub_rows"] and hs["out_hub_rows"] and hs["fwd"] == 2 and hs["src"] == 2 and hs == off[r][3], (r, hs)
        li, lo = _local_entries(da, gs[r])               # (the copies are built when the switch is set; no pass uses them)
        assert k0[r] == ZERO and k1[r] == dict(ZERO, hub_fallbacks=4, in_local_entries=li, out_local_entries=lo), (r, k1[r])


# ---- 7. the wide bf16 switch ----------------------------------------------------------------------------------------------------------------
def test_the_wide_bf16_form_is_not_taken(da):
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 2)
    gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
    dims, heads = [24, 128, 6], [8, 1]                         # (a shape of the wide form on the hidden layer)
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    opts = {"gatmh_bf16_gather": 2}

    def bf(wide):
        def f(ctx):
            ctx.gatmh_row_gather_bf16(1)
            ctx.gatmh_row_gather_bf16_wide(wide)
        return f
    narrow, kn = _run(da, gs, parts, X, labels, params, dims, heads, 1, opts, bf(0))
    wide, kw = _run(da, gs, parts, X, labels, params, dims, heads, 1, opts, bf(1))
    _same(narrow, wide, "wide not taken")
    for r in range(2):
        assert kn[r]["wide_not_taken"] == 0 and kw[r]["wide_not_taken"] == 4 and kw[r]["fwd_split"] == 2 and kw[r]["src_split"] == 2, (r, kn[r], kw[r])


# ---- 8. the epoch graph -------------------------------------------------------------------------------------------------------------------
def test_replayed_epochs_are_bit_identical_to_eager(da):
    """one rank's partition on a one-node context (an epoch graph records single partitions; the ghost rows stay as they are), mode 1,
    value 1: the first, eager epoch builds the copy, the recording finds it; two replayed epochs equal the eager ones"""
    import partition_oracle as po
    from test_gpu_gatmh_bf16_gather import make_gatmh
    s, d, parts, rng, _ = _block_graph(da, 2)
    g = po.preprocess(s, d, parts, 0, 2)
    dims, heads = [24, 64, 6], [4, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    states = []
    for graph in (0, 1):
        ctx = make_gatmh(da, g, dims, heads, len(parts), X[g["localToGlobal"]], labels[g["localToGlobal"]], params, {"gatmh_sweep": 0})
        try:
            ctx.gatmh_row_gather(1)
            ctx.gatmh_row_gather_edge_split(1)
            ctx.adam_config(0.01)
            ctx.set_option("epoch_graph", graph)
            eng = da.NativeEngine(ctx)
            eng.run(2)                                   # graph: one eager epoch, one recording
            eng.run(2)                                   # graph: two replays
            st = ctx.gatmh_row_gather_edge_split_stats()
            if graph:
                assert ctx.get_option("epoch_graph_recorded") == 1
                assert (st["fwd_split"], st["src_split"]) == (4, 4), st
            else:
                assert (st["fwd_split"], st["src_split"]) == (8, 8), st
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
        assert np.array_equal(_bits(states[0][k]), _bits(states[1][k])), k


# ---- 9. two runs ------------------------------------------------------------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(da):
    import partition_oracle as po
    s, d, parts, rng, _ = _block_graph(da, 3)
    gs = [po.preprocess(s, d, parts, r, 3) for r in range(3)]
    dims, heads = [24, 64, 6], [32, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    a, _ = _run(da, gs, parts, X, labels, params, dims, heads, 2)
    b, _ = _run(da, gs, parts, X, labels, params, dims, heads, 2)
    _same(a, b, "two runs")
    fa, _ = _epochs(da, 2, 1, 1)
    fb, _ = _epochs(da, 2, 1, 1)
    _same_run(fa, fb, "two runs in flight")


# ---- 10. refusals -----------------------------------------------------------------------------------------------------------------------------
def test_refusals_on_a_live_context(da):
    import partition_oracle as po
    for gnn in (da.GCN, da.GAT):
        c = da.Context(0)
        try:
            c.configure(gnn, [4, 16, 2], 100, 0, 2)
            for v in (1, 2):
                with pytest.raises(da.DoryError, match="gatmh_row_gather_edge_split.*DORY_GATMH"):
                    c.gatmh_row_gather_edge_split(v)
            c.gatmh_row_gather_edge_split(0)
        finally:
            c.close()
    s, d, parts, rng, _ = _block_graph(da, 2)
    g = po.preprocess(s, d, parts, 0, 2)
    dims, heads = [24, 128, 6], [8, 1]
    X, labels, params = _inputs(rng, len(parts), dims, heads)
    ctx = da.Context(0)
    try:
        ctx.configure(da.GATMH, dims, len(parts))
        ctx.gatmh_heads(heads)
        ctx.gatmh_row_gather(1)
        for bad in (3, -1):
            with pytest.raises(da.DoryError, match="gatmh_row_gather_edge_split: value .* is neither 0, 1 nor 2"):
                ctx.gatmh_row_gather_edge_split(bad)
        ctx.gatmh_row_gather_edge_split(1)               # before the graph: the first pass builds the copy
        ctx.graph_upload(g)
        ctx.preallocate()
        assert ctx.gatmh_row_gather_edge_split_stats() == ZERO
        ctx.upload(0, "h", X[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_edge(1, da.FORWARD)
        ctx.epoch_graph_begin()                          # a recording whose first use would have to build the copy
        try:
            with pytest.raises(da.DoryError, match="run one eager epoch first"):
                ctx.aggregate(1, da.FORWARD)
            for v in (0, 1, 2):
                with pytest.raises(da.DoryError, match="gatmh_row_gather_edge_split: not while an epoch graph is being recorded"):
                    ctx.gatmh_row_gather_edge_split(v)
        finally:
            ctx.epoch_graph_drop()
        assert ctx.gatmh_row_gather_edge_split_stats() == ZERO
        ctx.aggregate(1, da.FORWARD)                     # eager: builds the copy of the in-edges and runs the carry kernel
        li, lo = _local_entries(da, g)
        assert ctx.gatmh_row_gather_edge_split_stats() == dict(ZERO, fwd_split=1, in_local_entries=li)
        ctx.gatmh_row_gather_edge_split(0)
        ctx.gatmh_row_gather_edge_split(2)               # with a graph: both copies at once
        st = ctx.gatmh_row_gather_edge_split_stats()
        assert (st["in_local_entries"], st["out_local_entries"]) == (li, lo), st
        ctx.graph_upload(g)                              # a new upload drops them
        st = ctx.gatmh_row_gather_edge_split_stats()
        assert (st["in_local_entries"], st["out_local_entries"]) == (0, 0), st
    finally:
        ctx.close()
