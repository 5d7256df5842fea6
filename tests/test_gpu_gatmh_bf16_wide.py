"""Option gatmh_bf16_wide (include/dorylus_hip.h): where an edge pass of the multi-head GAT runs on bf16 rows (option
gatmh_bf16_gather) of 128 floats or more with several heads of 16, 32 or 64 features, its gathers fetch eight features per lane
(16 bytes) on 16-lane groups (csrc/gat_mh_sweep.hip: gatmh_forward_sweep_bf16x8_kernel, gatmh_src_sweep_bf16x8_kernel).

The wide form keeps every sum in the narrow bf16 form's order, so what is pinned is equality of bits:
  * wide against narrow (gatmh_bf16_wide = 0), stage by stage, forward and backward, over every lanes-per-head count, two slabs,
    a half-empty slab, a wide last layer, a layer the option does not apply to, forced and automatic layouts;
  * wide against the fp32 kernels on host-rounded rows (the contract of gatmh_bf16_gather, helpers of
    tests/test_gpu_gatmh_bf16_gather.py), phases 1 + 2 against phase 0;
  * split rows and pieces, ghost rows (two launches), the local transport with overlap on and off, epoch-graph replays;
  * refusals and the read-only counters.
Every test reads gatmh_bf16_gathers_fwd_wide / gatmh_bf16_gathers_src_wide: a silent fall-back to the narrow form cannot pass."""
import numpy as np
import pytest

from test_gpu_gatmh_bf16_gather import (FWD_NAMES, Pair, _pair, _split_inputs, backward_takes_the_sweep_forms, counters, hub_graph,
                                        make_gatmh, make_params, same_bits, special_rows)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def wide_counters(ctx):
    return ctx.get_option("gatmh_bf16_gathers_fwd_wide"), ctx.get_option("gatmh_bf16_gathers_src_wide")


def _pad32(cols):
    return (cols + 31) // 32 * 32


def takes_the_wide_form(K, D):
    """the rule of the option: rows of 128 floats or more, several heads, 16 / 32 / 64 features per head"""
    return K > 1 and D in (16, 32, 64) and _pad32(K * D) >= 128


def _kd(dims, heads):
    """(heads, features per head) of the two layers: layer 0's dims[1] is the whole row, layer 1 has dims[2] per head"""
    return [(heads[0], dims[1] // heads[0]), (heads[1], dims[2])]


def wide_against_narrow(da, g, rng, dims, heads, V, options, mode=2):
    """contexts A (gatmh_bf16_wide = 1) and B (0), both with gatmh_bf16_gather = mode, on the same inputs with special_rows planted
    in z: forward, then backward, stage by stage -- identical bits everywhere.  Returns A's (narrow, wide) counters."""
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = make_params(rng, dims, heads)
    A = make_gatmh(da, g, dims, heads, V, X, labels, params, dict(options, gatmh_bf16_gather=mode, gatmh_bf16_wide=1))
    B = make_gatmh(da, g, dims, heads, V, X, labels, params, dict(options, gatmh_bf16_gather=mode, gatmh_bf16_wide=0))
    kd = _kd(dims, heads)

    def both(f):
        f(A)
        f(B)
    for l in range(2):
        both(lambda c: c.apply_vertex(l, da.FORWARD))
        z = special_rows(rng, B.download(l, "z"))
        both(lambda c: c.upload(l, "z", z))
        both(lambda c: c.apply_edge(l + 1, da.FORWARD))
        c0 = [counters(A), wide_counters(A), counters(B), wide_counters(B)]
        both(lambda c: c.aggregate(l + 1, da.FORWARD))
        c1 = [counters(A), wide_counters(A), counters(B), wide_counters(B)]
        w = 1 if takes_the_wide_form(*kd[l]) else 0
        assert c1[0][0] - c0[0][0] == 1 and c1[2][0] - c0[2][0] == 1, (l, c0, c1)          # both ran the bf16 forward pass
        assert c1[1][0] - c0[1][0] == w and c1[3] == (0, 0), (l, c0, c1)                   # A alone, where it applies, wide
        for nm in FWD_NAMES:
            assert same_bits(A.download(l, nm), B.download(l, nm)), (l, nm)
        nxt = (l + 1, "h") if l < 1 else (l, "logits")
        assert same_bits(A.download(*nxt), B.download(*nxt)), (l, nxt)
    both(lambda c: c.predict_gat(2))
    for l in (1, 0):
        # a layer whose backward leaves the sweep forms (a single narrow head) refuses value 2: its backward runs with 1 in both
        swept = mode >= 2 and backward_takes_the_sweep_forms(*kd[l])
        both(lambda c: c.set_option("gatmh_bf16_gather", mode if swept or mode < 2 else 1))
        c0 = [counters(A), wide_counters(A), counters(B), wide_counters(B)]
        both(lambda c: c.aggregate(l + 1, da.BACKWARD))
        c1 = [counters(A), wide_counters(A), counters(B), wide_counters(B)]
        both(lambda c: c.set_option("gatmh_bf16_gather", mode))
        w = 1 if (swept and takes_the_wide_form(*kd[l])) else 0
        assert c1[0][1] - c0[0][1] == (1 if swept else 0) and c1[2][1] - c0[2][1] == (1 if swept else 0), (l, c0, c1)
        assert c1[1][1] - c0[1][1] == w and c1[1][0] == c0[1][0] and c1[3] == (0, 0), (l, c0, c1)
        both(lambda c: c.apply_vertex(l, da.BACKWARD))
        for nm in ("dz", "del", "der", "t"):
            assert same_bits(A.download(l, nm), B.download(l, nm)), (l, nm)
        for nm in ("w", "a_l", "a_r"):
            assert same_bits(A.weight_grad_get(l, nm), B.weight_grad_get(l, nm)), (l, "grad", nm)
    out = counters(A), wide_counters(A)
    assert np.isfinite(A.download(0, "dz")).all()
    A.close()
    B.close()
    return out


# dims, heads, V, E.  The last layer of the fifth shape is the wide one: 8 heads x 16 logits, averaged -- dims[2] counts the logits
# PER HEAD (make_params, _pair), so its z is 8 x 16 = 128 floats wide
WIDE_SHAPES = [([40, 128, 41], [8, 1], 300, 4000),      # D = 16: two lanes per head; layer 1 is one head: not wide
               ([24, 128, 6], [4, 1], 200, 1500),       # D = 32: four lanes per head
               ([24, 256, 6], [4, 1], 170, 1200),       # D = 64: eight lanes per head, two slabs
               ([24, 192, 6], [12, 1], 170, 1200),      # D = 16, ld = 192: the second slab is half empty (lanes without a column, the K - 1 clamp)
               ([24, 32, 16], [4, 8], 200, 1500),       # the LAST layer is the wide one; layer 0 (4 heads x 8 on 16-lane slabs) is not
               ([24, 256, 9], [32, 1], 140, 1000)]      # D = 8: the option does not apply


@pytest.mark.parametrize("nb", [8, 0])
@pytest.mark.parametrize("dims,heads,V,E", WIDE_SHAPES)
def test_wide_equals_narrow_bit_for_bit(da, dims, heads, V, E, nb):
    if nb == 0:       # the automatic layout: a graph large enough to get a sweep layout (tests/test_gpu_gatmh_bf16_gather.py: _pair)
        V = 20000
        E = 13 * V
    g, rng = hub_graph(dims, V, E)
    kd = _kd(dims, heads)
    (fwd, src), (fwd_w, src_w) = wide_against_narrow(da, g, rng, dims, heads, V, {"spmm_blk_nb": nb})
    n_wide = sum(takes_the_wide_form(*x) for x in kd)
    assert fwd == 2 and fwd_w == n_wide, (fwd, fwd_w)
    assert src == sum(backward_takes_the_sweep_forms(*x) for x in kd) and src_w == n_wide, (src, src_w)   # (every wide layer's backward sweeps)
    assert n_wide == (0 if dims == [24, 256, 9] else 1)                                                    # (what the shapes were chosen for)


@pytest.mark.parametrize("dims,heads,V,E", [WIDE_SHAPES[0], WIDE_SHAPES[2]])
def test_wide_equals_fp32_on_host_rounded_rows(da, dims, heads, V, E):
    """the contract of gatmh_bf16_gather asserted for the wide form directly: context A (value 2, wide) against the fp32 kernels of
    context B on rows rounded on the host -- forward, backward in phases 1 and 2; phase 0 equals the two phases in turn"""
    rng = np.random.default_rng(dims[1])
    p, _ = _pair(da, dims, heads, V, E, 8, 2, plant=lambda z: special_rows(rng, z))
    p.A.set_option("gatmh_bf16_wide", 1)
    p.forward()
    phased = p.backward()
    n = p.src_passes
    assert counters(p.A) == (2, n) and wide_counters(p.A) == (1, 1) and counters(p.B) == (0, 0) and wide_counters(p.B) == (0, 0)
    for l in (1, 0):
        swept = backward_takes_the_sweep_forms(*p.kd[l])
        p.A.set_option("gatmh_bf16_gather", 2 if swept else 1)
        p.A.aggregate(l + 1, da.BACKWARD)
        p.A.apply_vertex(l, da.BACKWARD)
        for nm in ("dz", "del"):
            assert same_bits(p.A.download(l, nm), phased[l][nm]), (l, nm)
        for nm in ("w", "a_l", "a_r"):
            assert same_bits(p.A.weight_grad_get(l, nm), phased[l]["g_" + nm]), (l, nm)
    assert counters(p.A) == (2, 2 * n) and wide_counters(p.A) == (1, 2)
    p.close()


def test_split_rows_and_pieces(da):
    """the construction of tests/test_gpu_gatmh_bf16_gather.py::test_split_rows_and_pieces: a hub destination and a hub source are
    cut into pieces by the sweep layouts; the wide form's pieces land in the same slots and are combined in piece order"""
    import partition_oracle as po
    dims, heads, V, E = [40, 128, 41], [8, 1], 400, 6000
    rng = np.random.default_rng(5 + len(dims) + dims[1])
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:400] = 11
    s[400:800] = 29
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    assert np.diff(g["colPtr"].astype(np.int64)).max() >= 400 and np.diff(g["rowPtr"].astype(np.int64)).max() >= 400
    narrow, wide = wide_against_narrow(da, g, rng, dims, heads, V, {"spmm_blk_nb": 8})
    assert narrow == (2, 2) and wide == (1, 1)


def test_ghost_rows_two_launches(da):
    """rank 0 of a 2-way split in one context, ghost tensors uploaded by hand (tests/test_gpu_gatmh_bf16_gather.py): the wide
    passes run the local-source blocks, then the ghost blocks on the sums of the first launch"""
    dims, heads, V, s, d, parts, X, labels, params = _split_inputs(2)
    part = da.Partition.build(s, d, parts, 0, 2)
    g = part.view()
    N, Gs, Gd = int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
    assert Gs > 0 and Gd > 0
    l2g = np.asarray(g["localToGlobal"])
    rng = np.random.default_rng(3)
    widths = [dims[1], dims[2] * heads[1]]
    ghosts = {}
    for l in range(2):
        ghosts[(l, "fg_z")] = rng.standard_normal((Gs, widths[l])).astype(np.float32)
        ghosts[(l, "bg_do")] = (rng.standard_normal((Gd, widths[l])) * 0.1).astype(np.float32)
    mk = lambda: make_gatmh(da, None, dims, heads, V, X[l2g], labels[l2g], params, {"spmm_blk_nb": 8}, 0, 2, part, parts)
    A, B = mk(), mk()
    p = Pair(da, A, B, 2, ghosts=ghosts)
    A.set_option("gatmh_bf16_wide", 1)
    p.forward()
    # the wide pass gathered both source arrays: o of the wide layer depends on a ghost row
    o_before = A.download(0, "o")
    A.upload(0, "fg_z", ghosts[(0, "fg_z")] + np.float32(1.0))
    A.aggregate(1, da.FORWARD)
    assert not np.array_equal(A.download(0, "o"), o_before)
    A.upload(0, "fg_z", ghosts[(0, "fg_z")])
    A.aggregate(1, da.FORWARD)
    assert same_bits(A.download(0, "o"), o_before)
    assert wide_counters(A) == (3, 0)
    p.backward(ghost_stats=rng.integers(0, N, Gd))
    assert counters(A) == (4, 2) and wide_counters(A) == (3, 1) and wide_counters(B) == (0, 0)
    p.close()


def test_local_transport_overlap_on_and_off_and_narrow_give_the_same_bits(da):
    """two ranks over the in-process device transport, three epochs in the Engine: wide with the exchange overlapped, wide without,
    and narrow -- the same bits in every downloaded tensor, weight and gradient"""
    from local_ranks import run_local
    P = 2
    dims, heads, V, s, d, parts, X, labels, params = _split_inputs(P)
    runs, counts = [], []
    for overlap, wide in ((1, 1), (0, 1), (1, 0)):
        seen = {}

        def setup(ctx, r, g):
            ctx.upload(0, "h", X[g["localToGlobal"]])
            ctx.labels_upload(labels[g["localToGlobal"]])
            for l, (W, al, ar) in enumerate(params):
                ctx.weight_set(l, "w", W)
                ctx.weight_set(l, "a_l", al)
                ctx.weight_set(l, "a_r", ar)
            close = ctx.close

            def close_and_count():                    # (run_local closes its contexts: read the counters just before)
                if r not in seen:
                    seen[r] = counters(ctx) + wide_counters(ctx) + (int(g["srcGhostCnt"]), int(g["dstGhostCnt"]))
                close()
            ctx.close = close_and_count
        pobjs = [da.Partition.build(s, d, parts, r, P) for r in range(P)]
        dl = [(l, nm) for l in range(2) for nm in ("z", "o", "op", "t", "del", "der", "dz")] + [(1, "logits")]
        runs.append(run_local(da, pobjs, parts, dims, da.GATMH, 3, setup,
                              {"spmm_blk_nb": 8, "halo_overlap": overlap, "gatmh_bf16_gather": 2, "gatmh_bf16_wide": wide}, downloads=dl,
                              pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r")))
        counts.append((wide, seen))
    for wide, seen in counts:
        assert len(seen) == P
        for r, (fwd, src, fwd_w, src_w, Gs, Gd) in seen.items():
            assert Gs > 0 and Gd > 0 and fwd == 6 and src == 6, (r, fwd, src, Gs, Gd)     # 3 epochs x 2 layers
            assert (fwd_w, src_w) == ((3, 3) if wide else (0, 0)), (r, wide, fwd_w, src_w)  # layer 0 of every epoch
    a = runs[0]
    for b in runs[1:]:
        for r in range(P):
            assert a["tensors"][r].keys() == b["tensors"][r].keys() and len(a["tensors"][r]) >= 15
            for k in a["tensors"][r]:
                assert same_bits(a["tensors"][r][k], b["tensors"][r][k]), (r, k)
            for l in range(2):
                for nm in ("w", "a_l", "a_r"):
                    assert same_bits(a["weights"][r][l][nm], b["weights"][r][l][nm]), (r, l, nm)
                    assert same_bits(a["wgrads"][r][l][nm], b["wgrads"][r][l][nm]), (r, l, nm)


def test_replayed_epochs_are_bit_identical_to_eager(da):
    """the pattern of tests/test_gpu_gatmh_bf16_gather.py::test_replayed_epochs_are_bit_identical_to_eager at a shape with a wide
    layer (8 heads x 16, then two heads of 8): ten epochs eager, ten with the epoch recorded and replayed, and ten in which the
    option is switched on between two recordings -- the wide counters tell the runs apart, no output bit does"""
    import partition_oracle as po
    V, E, dims, heads = 2708, 5278, [64, 128, 8], [8, 2]
    assert takes_the_wide_form(8, 16) and not takes_the_wide_form(2, 8) and backward_takes_the_sweep_forms(2, 8)
    states = []
    for graph, first in ((0, 1), (1, 1), (1, 0)):
        rng = np.random.default_rng(5)
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
        g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.fill_uniform(0, "h", 3, -1.0, 1.0, g["localToGlobal"])
        ctx.labels_upload(rng.integers(0, 7, V).astype(np.uint32))
        ctx.weights_init_xavier()
        ctx.adam_config(0.01)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.set_option("gatmh_bf16_wide", first)
        ctx.set_option("epoch_graph", graph)
        eng = da.NativeEngine(ctx)
        eng.run(6)
        if not first:                           # narrow so far: drop the recording, switch the option on, record again
            assert ctx.get_option("epoch_graph_recorded") == 1
            assert counters(ctx) == (4, 4) and wide_counters(ctx) == (0, 0)
            ctx.epoch_graph_drop()
            ctx.set_option("gatmh_bf16_wide", 1)
        eng.run(4)
        if not first:                           # (after the drop: one eager epoch and one recording again)
            assert ctx.get_option("epoch_graph_recorded") == 1
            assert counters(ctx) == (8, 8) and wide_counters(ctx) == (2, 2)
        elif graph:                             # one eager epoch and one recording: replays do not count
            assert ctx.get_option("epoch_graph_recorded") == 1
            assert counters(ctx) == (4, 4) and wide_counters(ctx) == (2, 2)
        else:
            assert counters(ctx) == (20, 20) and wide_counters(ctx) == (10, 10)
        st = {}
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                st[(nm, l)] = ctx.weight_get(l, nm)
                st[("d" + nm, l)] = ctx.weight_grad_get(l, nm)
            for nm in ("z", "o", "op", "dz", "el", "t", "del"):
                st[(nm, l)] = ctx.download(l, nm)
        states.append(st)
        eng.close()
        ctx.close()
    for other in states[1:]:
        for k in states[0]:
            assert same_bits(states[0][k], other[k]), k


def test_refusals_and_read_only_keys(da):
    for gnn in (da.GCN, da.GAT):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        with pytest.raises(da.DoryError):
            ctx.set_option("gatmh_bf16_wide", 1)
        ctx.set_option("gatmh_bf16_wide", 0)
        assert ctx.get_option("gatmh_bf16_wide") == 0
        ctx.close()
    ctx = da.Context(0)                       # set on a fresh context, then configured as GCN: refused there
    ctx.set_option("gatmh_bf16_wide", 1)
    with pytest.raises(da.DoryError):
        ctx.configure(da.GCN, [16, 8, 3], 100)
    ctx.close()

    dims, heads, V, E = [40, 128, 41], [8, 1], 300, 4000
    g, rng = hub_graph(dims, V, E)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    ctx = make_gatmh(da, g, dims, heads, V, X, labels, make_params(rng, dims, heads), {"spmm_blk_nb": 8})
    assert ctx.get_option("gatmh_bf16_wide") == 0 and wide_counters(ctx) == (0, 0)
    for bad in (2, -1):
        with pytest.raises(da.DoryError):
            ctx.set_option("gatmh_bf16_wide", bad)
        assert ctx.get_option("gatmh_bf16_wide") == 0
    for key in ("gatmh_bf16_gathers_fwd_wide", "gatmh_bf16_gathers_src_wide"):
        with pytest.raises(da.DoryError):
            ctx.set_option(key, 1)                               # the counters are read-only
    ctx.set_option("gatmh_bf16_wide", 1)

    def epoch():
        for l in range(2):
            ctx.apply_vertex(l, da.FORWARD)
            ctx.apply_edge(l + 1, da.FORWARD)
            ctx.aggregate(l + 1, da.FORWARD)
        ctx.predict_gat(2)
        for l in (1, 0):
            ctx.aggregate(l + 1, da.BACKWARD)
            ctx.apply_vertex(l, da.BACKWARD)
        ctx.sync()
        return [ctx.download(0, nm) for nm in ("o", "dz")]
    # without bf16 rows the option changes nothing: the fp32 kernels run, every bf16 counter stays 0
    ctx.set_option("gatmh_bf16_gather", 0)
    fp32 = epoch()
    assert counters(ctx) == (0, 0) and wide_counters(ctx) == (0, 0)
    ctx.set_option("gatmh_bf16_wide", 0)
    for a, b in zip(fp32, epoch()):
        assert same_bits(a, b)
    ctx.set_option("gatmh_bf16_wide", 1)
    # value 1: the forward runs wide, the backward's source side runs in fp32
    ctx.set_option("gatmh_bf16_gather", 1)
    one = epoch()
    assert counters(ctx) == (2, 0) and wide_counters(ctx) == (1, 0)
    assert not np.array_equal(one[0], fp32[0])                   # (the rows were rounded)
    ctx.set_option("gatmh_bf16_gather", 2)
    epoch()
    assert counters(ctx) == (4, 2) and wide_counters(ctx) == (2, 1)
    ctx.close()
