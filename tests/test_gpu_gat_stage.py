"""The reference GAT prototype's own stage, kernel by kernel, against float64 numpy (tests/gat_stage_ref.py):
edge_forward_gat_kernel / edge_backward_gat_kernel, expand_rows_to_edges_kernel, colsum_w -> rowdot -> colsum_w (the a_i
gradient), row_axpy_kernel and the three ways aggregate_gat forms one ah / aTg, plus the cached per-destination state between
the stages -- every stage driven through the public ABI on its OWN uploaded inputs, so that nothing propagates from one stage
into the next.

Two input families (gat_stage_ref.stage_inputs): dyadic inputs, whose dot products are exact in fp32 in any order -- az, A,
azrow, arow, cw and every sign have to be the reference's bits -- and random inputs, judged element by element against the
bound derived from the float64 magnitudes of the same inputs (|got - ref| / bound <= 1; the worst ratio of every check is
printed before it is asserted: run with -s to read them).  The premises -- the case list reaches every class, no random
column is near LeakyReLU's edge, every plausible kernel mistake would show at ten times the bound -- are checked without a GPU
by tests/test_gat_stage_reference.py."""
import numpy as np
import pytest

import gat_stage_ref as gr
from gat_stage_ref import EDGE_IDS, golden, golden_parts, graph

pytestmark = pytest.mark.gpu

FWD, BWD = 0, 1
LAUNCH_KEYS = ("spmm_launches_k1s", "spmm_launches_k1b", "spmm_launches_k1")
# the three ways of one aggregation: options, and what the launch counters have to show
WAYS = {"k1": dict(spmm_blk_nb=0, gat_reuse_nsum=0), "unit": dict(spmm_blk_nb=8, gat_reuse_nsum=0), "nsum": dict(spmm_blk_nb=8, gat_reuse_nsum=1)}


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a, b):
    a, b = np.ascontiguousarray(a, np.float32).reshape(-1), np.ascontiguousarray(b, np.float32).reshape(-1)
    return a.size == b.size and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _ratio(what, got, ref, bound):
    """max |got - ref| / bound, printed, then asserted"""
    assert np.isfinite(np.asarray(got)).all(), what
    q = gr.err_over_bound(np.asarray(got, np.float64).reshape(np.shape(ref)), ref, bound)
    print("ratio", what, f"{q:.4g}")
    assert q <= 1.0, (what, q)
    return q


def _make(da, g, dims, options, r=0, P=1):
    from helpers import make_ctx
    return make_ctx(da, g, dims, g["globalVtxCnt"], gnn=da.GAT, node_id=r, num_nodes=P, options=options)


def _up(ctx, layer, name, a):
    if np.size(a):
        ctx.upload(layer, name, a)


def _poison(ctx, layer, names):
    from helpers import _poison_padding
    return sum(_poison_padding(ctx, layer, n) for n in names)


def _launches(ctx):
    return np.array([ctx.get_option(k) for k in LAUNCH_KEYS])


def _per_vertex(z, a):
    """the edge forward's per-destination values, deg-0 vertices included: one virtual edge per vertex"""
    return gr.edge_forward(np.arange(z.shape[0] + 1), z, a)


# ---- edge forward / backward over the case list ---------------------------------------------------------------------------
def _edge_stage(da, g, F, fam, lazy):
    what = (g["localVtxCnt"], F, fam, "lazy" if lazy else "eager")
    cp = g["colPtr"]
    inp = gr.stage_inputs(g, F, fam)
    ctx = _make(da, g, [8, F], {"gat_lazy_edge_tensors": lazy})
    ctx.upload(0, "z", inp["z"])
    ctx.upload(0, "grad", inp["grad"])
    ctx.weight_set(0, "a_i", inp["a"])
    out = []
    for poisoned in (False, True):      # padding columns of z / grad are NaN the second time: nothing may change
        if poisoned:
            assert _poison(ctx, 0, ["z", "grad"]) > 0 or F % 32 == 0 or F == 1      # (rows are padded to 32 floats; one column is not padded)
        ctx.apply_edge(1, FWD)
        fwd = {nm: ctx.download(0, nm).ravel() for nm in ("azrow", "arow", "az", "A")}
        ctx.apply_edge(1, BWD)
        bwd = {nm: ctx.download(0, nm).ravel() for nm in ("drow", "dA", "cw")}
        bwd["da"] = ctx.weight_grad_get(0, "a_i").ravel()
        out.append({**fwd, **bwd})
    for nm, v in out[0].items():
        assert _bits(v, out[1][nm]), what + (nm, "NaN in the padding columns changed it")
    o = out[0]
    # forward: the per-destination values against the reference of every vertex, the per-edge tensors against the per-edge
    # reference and, edge for edge, equal to the per-destination values (expand_rows_to_edges_kernel when lazy)
    pv, fw = _per_vertex(inp["z"], inp["a"]), gr.edge_forward(cp, inp["z"], inp["a"])
    assert _bits(o["az"], gr.expand_rows(cp, o["azrow"])) and _bits(o["A"], gr.expand_rows(cp, o["arow"])), what + ("expand",)
    if fam == "dyadic":
        for got, ref, nm in ((o["azrow"], pv["az"], "azrow"), (o["arow"], pv["A"], "arow"), (o["az"], fw["az"], "az"), (o["A"], fw["A"], "A")):
            assert _bits(got, ref.astype(np.float32)), what + (nm, "bits")
    else:
        _ratio(what + ("azrow",), o["azrow"], pv["az"], pv["b_az"])
        _ratio(what + ("arow",), o["arow"], pv["A"], pv["b_A"])
        _ratio(what + ("az",), o["az"], fw["az"], fw["b_az"])
        _ratio(what + ("A",), o["A"], fw["A"], fw["b_A"])
    # the branch of every column, none excluded (the margin of the random inputs is a premise, test_gat_stage_reference.py)
    assert np.array_equal(o["azrow"] > 0, pv["az"] > 0) and np.array_equal(o["azrow"] == 0, pv["az"] == 0), what + ("signs",)
    assert not np.signbit(o["azrow"][pv["az"] == 0]).any() and not np.signbit(o["arow"][pv["az"] == 0]).any(), what + ("az = +0",)
    _edge_backward_checks(what + ("computed az",), g, inp, o, o["az"])
    # a caller's own az drives the backward: other signs than the computed ones, +0 and -0.0 among them (premises of the case
    # list, test_case_list_covers_the_classes).  The forward runs again first and nothing is read in between: when lazy, the
    # upload meets an az whose expansion is still pending, and that expansion must not land on the caller's values later
    ctx.apply_edge(1, FWD)
    _up(ctx, 0, "az", inp["az_up"])
    ctx.apply_edge(1, BWD)
    assert _bits(ctx.download(0, "az"), inp["az_up"]), what + ("the caller's az is still there",)
    o2 = {nm: ctx.download(0, nm).ravel() for nm in ("drow", "dA", "cw")}
    o2["da"] = ctx.weight_grad_get(0, "a_i").ravel()
    _edge_backward_checks(what + ("uploaded az",), g, inp, o2, inp["az_up"])
    ctx.close()


def _edge_backward_checks(what, g, inp, o, az):
    cp, deg = g["colPtr"], gr.in_degrees(g)
    bw = gr.edge_backward(cp, inp["grad"], az, inp["z"], inp["a"])
    assert _bits(o["dA"], gr.expand_rows(cp, o["drow"])), what + ("dA is drow expanded",)
    assert _bits(o["cw"], bw["cw"].astype(np.float32)), what + ("cw bits",)        # deg * s_v: one rounding of an exact product
    assert not o["cw"][deg == 0].any() and not o["drow"][deg == 0].any(), what + ("a vertex without in-edges",)
    _ratio(what + ("dA",), o["dA"], bw["dA"], bw["b_dA"])
    if what[2] == "dyadic":      # on the branch of slope 1 nothing is rounded
        assert _bits(o["dA"][bw["dl"] == 1], bw["dA"][bw["dl"] == 1].astype(np.float32)), what + ("dA bits",)
    _ratio(what + ("da",), o["da"], bw["da"], bw["b_da"])


@pytest.mark.parametrize("N,F", gr.EDGE_CASES, ids=EDGE_IDS)
def test_edge_stage(da, N, F):
    """edge forward and backward of one (N, F): both families, per-edge tensors written eagerly and on demand"""
    for fam in gr.FAMILIES:
        for lazy in (0, 1):
            _edge_stage(da, graph(N), F, fam, lazy)


def test_width_one(da):
    """F = 1, recorded: tensors of one column keep ld = 1.  The edge stage works on them (element loads; checked like every
    other width); the aggregations are refused with an error code -- K1 gathers 16-byte pieces -- and launch nothing."""
    N, F = gr.WIDTH_ONE
    g = graph(N)
    for fam in gr.FAMILIES:
        _edge_stage(da, g, F, fam, 1)
    inp = gr.stage_inputs(g, F, "random")
    for way, opts in WAYS.items():
        ctx = _make(da, g, [8, F], opts)
        assert ctx.info(0, "z")[2] == 1
        ctx.upload(0, "z", inp["z"])
        ctx.upload(0, "grad", inp["grad"])
        ctx.weight_set(0, "a_i", inp["a"])
        ctx.apply_edge(1, FWD)
        ctx.apply_edge(1, BWD)
        mark = np.full((N, F), 5.0, np.float32)
        for name, d in (("ah", FWD), ("aTg", BWD)):
            ctx.upload(0, name, mark)
            with pytest.raises(da.DoryError):
                ctx.aggregate(1, d)
            assert _bits(ctx.download(0, name), mark), (way, name)
        ctx.close()


# ---- one aggregation, three ways ------------------------------------------------------------------------------------------
def _agg_partitions():
    out = [(f"N{N}-F{F}", graph(N), F, 0, 1) for N, F in gr.AGG_CASES]
    for name, F in gr.AGG_GOLDENS:
        gs = golden(name)
        out += [(f"{name}-r{r}-F{F}", g, F, r, len(gs)) for r, g in enumerate(gs)]
    return out


AGG_PARTS = _agg_partitions()


def _expect_path(what, way, before, after, n_aggregations):
    """which kernels ran, from the launch counters: K1 alone, or the unit-weight layouts (K1s / K1b) alone; the unit way gathers
    once per aggregation, the nsum way once per aggregation that is not a row scaling of the kept sum; no stray gather"""
    k1s, k1b, k1 = (after - before).tolist()
    if way == "k1":
        assert k1 == n_aggregations and k1s == k1b == 0, what + ("launches", k1s, k1b, k1)
    else:
        assert k1 == 0 and k1s + k1b == n_aggregations, what + ("launches", k1s, k1b, k1)


def _aggregate_three_ways(da, label, g, F, r, P, way, lazy, fam):
    what = (label, way, "lazy" if lazy else "eager", fam)
    inp = gr.stage_inputs(g, F, fam)
    ctx = _make(da, g, [8, F], dict(WAYS[way], gat_lazy_edge_tensors=lazy), r, P)
    for nm in ("z", "fg_z", "grad", "bg_d"):
        _up(ctx, 0, nm, inp[nm])
    ctx.weight_set(0, "a_i", inp["a"])
    _poison(ctx, 0, ["ah", "aTg", "nsum"])       # outputs: whatever the padding holds, the kernels write whole rows or leave it alone
    ctx.apply_edge(1, FWD)
    c0 = _launches(ctx)
    ctx.aggregate(1, FWD)
    c1 = _launches(ctx)
    _expect_path(what + ("forward",), way, c0, c1, 1)
    A = ctx.download(0, "A").ravel()              # what the caller can see
    assert _bits(A, gr.expand_rows(g["colPtr"], ctx.download(0, "arow")))
    ah, b = gr.aggregate_fwd(g, A, inp["z"], inp["fg_z"])
    _ratio(what + ("ah",), ctx.download(0, "ah"), ah, b)
    if way == "nsum":
        S, b = gr.neighbour_sum(g, inp["z"], inp["fg_z"])
        q = _ratio(what + ("nsum",), ctx.download(0, "nsum"), S, b)
        if fam == "dyadic":
            assert q == 0.0, what + ("nsum of dyadic rows is exact",)
    ctx.apply_edge(1, BWD)
    c2 = _launches(ctx)
    ctx.aggregate(1, BWD)
    # the nsum way: A^T grad gathers, dA Z is drow * nsum (row_axpy_kernel) -- one launch instead of two
    _expect_path(what + ("backward",), way, c2, _launches(ctx), 1 if way == "nsum" else 2)
    dA = ctx.download(0, "dA").ravel()
    aTg, b = gr.aggregate_bwd(g, inp["grad"], inp["bg_d"], dA, inp["z"], inp["fg_z"])
    _ratio(what + ("aTg",), ctx.download(0, "aTg"), aTg, b)
    ctx.close()


@pytest.mark.parametrize("lazy", [0, 1], ids=["eager", "lazy"])
@pytest.mark.parametrize("way", list(WAYS))
@pytest.mark.parametrize("case", range(len(AGG_PARTS)), ids=[p[0] for p in AGG_PARTS])
def test_aggregation_three_ways(da, case, way, lazy):
    """ah, nsum and aTg of one partition against float64 and the derived bound: K1 on the per-edge values, the unit-weight
    gather with the row scale, and the kept neighbour sum with row_axpy_kernel -- which of them ran is read off the launch
    counters; graphs with the pinned in-degrees and the hub, and every rank of the two goldens with ghost rows"""
    label, g, F, r, P = AGG_PARTS[case]
    for fam in gr.FAMILIES:
        _aggregate_three_ways(da, label, g, F, r, P, way, lazy, fam)


# ---- the open case: parts_toy60_p4_hash ---------------------------------------------------------------------------------------
def test_open_case_p4_hash_per_stage(da):
    """parts_toy60_p4_hash, every rank, both layers of dims [20, 16, 6]: each stage gets the fp32 inputs the C oracle's epoch
    gave it and is compared with the float64 stage of those inputs.  The epoch tests dropped this graph because the GPU's aTg@0
    missed the suite's element-wise criterion 2.57 times; the oracle's own epoch misses it too
    (test_fp32_oracle_epoch_misses_the_elementwise_criterion_on_p4_hash).  Taken per stage every tensor, aTg@0 included, has
    to sit inside the derived bound; the four numbers of aTg@0 (GPU and C oracle, in units of the bound and of
    helpers.elem_err) are printed for profiles/HISTORY.md."""
    from helpers import elem_err, oracle_gat_epoch_parts
    OPEN_CASE, OPEN_DIMS = gr.OPEN_CASE, gr.OPEN_DIMS
    gs, parts, H0, labels, Ws, As = gr.open_case_inputs()
    T32, _, _ = oracle_gat_epoch_parts(gs, parts, H0, labels, Ws, As)
    worst = {}
    for nb in (0, 8):
        for r, g in enumerate(gs):
            t = T32[r]
            ctx = _make(da, g, OPEN_DIMS, {"spmm_blk_nb": nb}, r, len(gs))
            for l in range(2):
                what = (OPEN_CASE, nb, r, l)
                for nm in ("z", "fg_z", "grad", "bg_d"):
                    _up(ctx, l, nm, t[f"{nm}{l}"])
                ctx.weight_set(l, "a_i", As[l])
                ctx.apply_edge(l + 1, FWD)
                fw = gr.edge_forward(g["colPtr"], t[f"z{l}"], As[l])
                az, A = ctx.download(l, "az").ravel(), ctx.download(l, "A").ravel()
                _ratio(what + ("az",), az, fw["az"], fw["b_az"])
                _ratio(what + ("A",), A, fw["A"], fw["b_A"])
                assert np.array_equal(az > 0, fw["az"] > 0), what
                ctx.aggregate(l + 1, FWD)
                ah, b = gr.aggregate_fwd(g, A, t[f"z{l}"], t[f"fg_z{l}"])
                _ratio(what + ("ah",), ctx.download(l, "ah"), ah, b)
                ctx.apply_edge(l + 1, BWD)
                bw = gr.edge_backward(g["colPtr"], t[f"grad{l}"], az, t[f"z{l}"], As[l])
                dA = ctx.download(l, "dA").ravel()
                _ratio(what + ("dA",), dA, bw["dA"], bw["b_dA"])
                _ratio(what + ("da",), ctx.weight_grad_get(l, "a_i").ravel(), bw["da"], bw["b_da"])
                ctx.aggregate(l + 1, BWD)
                got = ctx.download(l, "aTg")
                aTg, b = gr.aggregate_bwd(g, t[f"grad{l}"], t[f"bg_d{l}"], dA, t[f"z{l}"], t[f"fg_z{l}"])
                q = _ratio(what + ("aTg",), got, aTg, b)
                if l == 0:
                    o_aTg, o_b = gr.aggregate_bwd(g, t["grad0"], t["bg_d0"], t["dA0"], t["z0"], t["fg_z0"])
                    for k, v in ((("gpu", nb, "bound"), q), (("gpu", nb, "elem_err"), elem_err(got, aTg)),
                                 (("oracle", "bound"), gr.err_over_bound(t["aTg0"], o_aTg, o_b)), (("oracle", "elem_err"), elem_err(t["aTg0"], o_aTg))):
                        worst[k] = max(worst.get(k, 0.0), v)
            ctx.close()
    print("open case aTg@0, worst rank:", {" ".join(map(str, k)): float(f"{v:.4g}") for k, v in worst.items()})
    assert worst[("oracle", "bound")] <= 1.0


# ---- cached state between the stages ------------------------------------------------------------------------------------------
CACHE_CASE, CACHE_RANK, CACHE_DIMS = "parts_toy60_p2", 0, [8, 16, 6]
ACTIONS = (["upload " + nm for nm in ("A", "dA", "az", "z", "fg_z")] + ["fill " + nm for nm in ("A", "dA", "az", "z", "fg_z")] +
           ["halo_unpack", "halo_unpack_tensor fg_z", "apply_vertex forward", "apply_edge forward of the next layer"])
FIRST_CALLS = ["aggregate forward", "aggregate backward", "apply_edge backward"]


def _cache_ctx(da, nb, lazy):
    """a context of two layers whose layer-0 stages have all run once: arow / drow / azrow / nsum describe the tensors"""
    from halo_plan_ref import halo_plan
    gs = golden(CACHE_CASE)
    parts = golden_parts(CACHE_CASE)
    g = gs[CACHE_RANK]
    ctx = _make(da, g, CACHE_DIMS, {"spmm_blk_nb": nb, "gat_lazy_edge_tensors": lazy}, CACHE_RANK, len(gs))
    pl = halo_plan(g, parts, CACHE_RANK, len(gs))
    for d in (0, 1):
        ctx.halo_plan(d, pl[d][0], pl[d][1])
    rng = np.random.default_rng(5)
    N = g["localVtxCnt"]
    ctx.upload(0, "h", rng.uniform(-1, 1, (N, CACHE_DIMS[0])).astype(np.float32))
    ctx.weight_set(0, "w", (rng.standard_normal((CACHE_DIMS[0], CACHE_DIMS[1])) / 3).astype(np.float32))
    for l in range(2):
        inp = gr.stage_inputs(g, CACHE_DIMS[l + 1], "random", seed=l)
        for nm in ("z", "fg_z", "grad", "bg_d"):
            _up(ctx, l, nm, inp[nm])
        ctx.weight_set(l, "a_i", inp["a"])
    for _ in range(2):        # twice: the second pass runs with every cache valid
        ctx.apply_edge(1, FWD)
        ctx.aggregate(1, FWD)
        ctx.apply_edge(1, BWD)
        ctx.aggregate(1, BWD)
    return ctx, g


def _visible(ctx, l=0):
    t = {nm: ctx.download(l, nm) for nm in ("z", "fg_z", "grad", "bg_d")}
    t.update({nm: ctx.download(l, nm).ravel() for nm in ("az", "A", "dA")})
    t["a"] = ctx.weight_get(l, "a_i")
    return t


def _raw_upload(ctx, layer, name, a):
    """dory_tensor_upload itself.  Context.upload asks dory_tensor_info for the shape first, and a raw pointer to a per-edge
    tensor makes the library write a pending expansion out: through it an upload would never meet one."""
    from dorylus_amd._lib import _ptr
    a = np.ascontiguousarray(a, np.float32)
    ctx._ck(ctx.lib.dory_tensor_upload(ctx.h, layer, name.encode(), _ptr(a)))


def _act(ctx, g, action, rng, like, vary_az=False):
    """the caller's action (`like`: the tensors' shapes); returns what it wrote where that has to be readable afterwards"""
    import torch
    from helpers import splitmix_uniform
    kind, _, name = action.partition(" ")
    if kind == "upload":
        a = rng.uniform(-1, 1, like[name].shape).astype(np.float32)
        if name == "az" and not vary_az:      # one value per destination, as every az the stage computes
            a = gr.expand_rows(g["colPtr"], rng.uniform(-1, 1, g["localVtxCnt"]).astype(np.float32))
        _raw_upload(ctx, 0, name, a)
        return name, a
    if kind == "fill":
        ctx.fill_uniform(0, name, 77, -1.0, 1.0)
        shape = like[name].shape if like[name].ndim == 2 else (like[name].size, 1)
        return name, splitmix_uniform(77, np.arange(shape[0]), shape[1])
    if kind in ("halo_unpack", "halo_unpack_tensor"):
        rows, cols, ld, _ = ctx.info(0, "fg_z")
        buf = np.zeros((rows, ld), np.float32)
        buf[:, :cols] = rng.uniform(-1, 1, (rows, cols))
        dev = torch.from_numpy(buf).cuda()
        torch.cuda.synchronize()
        if kind == "halo_unpack":
            ctx.halo_unpack(1, FWD, dev.data_ptr())
        else:
            ctx.halo_unpack_tensor(0, "fg_z", FWD, dev.data_ptr())
        ctx.sync()
        # received row k of peer p lands in the k-th ghost slot p owns: with one peer, in slot order
        return "fg_z", buf[:, :cols]
    if action == "apply_vertex forward":
        ctx.apply_vertex(0, FWD)
        return None, None
    assert action == "apply_edge forward of the next layer"
    ctx.apply_edge(2, FWD)          # "A" now holds layer 1's scores, and only those
    return None, None


ORDERS = ["read, then call", "call, then read"]


def _primed_snapshot(da, nb, lazy):
    """what a caller would download from a primed context -- taken from a TWIN, because a download writes the pending per-edge
    expansions out (gat_lazy_edge_tensors): the context under test meets the action with az / A / dA still pending"""
    twin, _ = _cache_ctx(da, nb, lazy)
    t = _visible(twin)
    twin.close()
    return t


def _after_action(da, action, nb, lazy, first, order, before, vary_az=False):
    """one context: primed, the action, then `first` -- before or after the caller reads the tensors back.  Returns the context,
    the graph, what the caller sees (read where `order` says) and the tag of the assertions"""
    ctx, g = _cache_ctx(da, nb, lazy)
    what = (action, nb, lazy, first, order)
    name, wrote = _act(ctx, g, action, np.random.default_rng(9), before, vary_az)
    call = {"aggregate forward": lambda: ctx.aggregate(1, FWD), "aggregate backward": lambda: ctx.aggregate(1, BWD),
            "apply_edge backward": lambda: ctx.apply_edge(1, BWD)}[first]
    if order == "call, then read":
        call()
    v = _visible(ctx)
    rewritten = "dA" if first == "apply_edge backward" and order == "call, then read" else None
    if name is not None and name != rewritten:
        assert _bits(v[name], wrote), what + (name, "what the caller wrote is not what it reads back")
    for nm in before:
        if nm not in (name, rewritten) and not (nm == "z" and action == "apply_vertex forward") and not (nm == "A" and "next layer" in action):
            assert _bits(v[nm], before[nm]), what + (nm, "changed by an action on another tensor")
    if "next layer" in action:
        assert _bits(v["A"], gr.expand_rows(g["colPtr"], ctx.download(1, "arow"))) and not _bits(v["A"], before["A"]), what
    if order == "read, then call":
        call()
        after = _visible(ctx)
        for nm in ("z", "fg_z", "grad", "bg_d", "az", "A") + (("dA",) if first != "apply_edge backward" else ()):
            assert _bits(after[nm], v[nm]), what + (nm, "a stage rewrote a tensor it only reads")
    return ctx, g, v, what


def _check_edge_backward(ctx, g, v, az, what):
    bw = gr.edge_backward(g["colPtr"], v["grad"], az, v["z"], v["a"])
    _ratio(what + ("dA",), ctx.download(0, "dA").ravel(), bw["dA"], bw["b_dA"])
    assert _bits(ctx.download(0, "cw"), bw["cw"].astype(np.float32)), what + ("cw",)
    _ratio(what + ("da",), ctx.weight_grad_get(0, "a_i").ravel(), bw["da"], bw["b_da"])


@pytest.mark.parametrize("lazy", [0, 1], ids=["eager", "lazy"])
@pytest.mark.parametrize("nb", [0, 8], ids=["k1", "blocked"])
@pytest.mark.parametrize("action", ACTIONS, ids=[a.replace(" ", "_") for a in ACTIONS])
def test_cached_state_follows_the_caller(da, action, nb, lazy):
    """after a caller's action the next aggregation or backward edge pass computes from what the caller can SEE -- the
    downloaded per-edge tensors and the current z / fg_z -- not from a per-destination value or a neighbour sum kept from
    before: float64 of the downloads, per-edge definition, derived bound.  Every action is followed by each of the three calls
    first (a forward aggregation refreshes what a backward one would reuse), each on a context whose caches were all valid and
    -- when lazy -- whose per-edge expansions are still pending when the action arrives; the caller reads the tensors back before
    the call, or only after it (then the call itself is the first to need the expansions)."""
    before = _primed_snapshot(da, nb, lazy)
    for first in FIRST_CALLS:
        if action == "fill az" and first == "apply_edge backward":
            continue      # az then varies within a destination: test_callers_az_is_read_at_the_first_in_edge has that pair
        for order in ORDERS:
            ctx, g, v, what = _after_action(da, action, nb, lazy, first, order, before)
            if first == "aggregate forward":
                ref, b = gr.aggregate_fwd(g, v["A"], v["z"], v["fg_z"])
                _ratio(what + ("ah",), ctx.download(0, "ah"), ref, b)
            elif first == "aggregate backward":
                ref, b = gr.aggregate_bwd(g, v["grad"], v["bg_d"], v["dA"], v["z"], v["fg_z"])
                _ratio(what + ("aTg",), ctx.download(0, "aTg"), ref, b)
            else:
                _check_edge_backward(ctx, g, v, v["az"], what)
            ctx.close()


@pytest.mark.parametrize("lazy", [0, 1], ids=["eager", "lazy"])
@pytest.mark.parametrize("nb", [0, 8], ids=["k1", "blocked"])
@pytest.mark.parametrize("action", ["upload az", "fill az"], ids=["upload", "fill"])
def test_callers_az_is_read_at_the_first_in_edge(da, action, nb, lazy):
    """pinned, and the one place where the float64 side is not the per-edge definition: the prototype's scores are per
    destination, and edge_backward_gat_kernel reads a caller's az at the FIRST in-edge of every destination.  An az that varies
    within a destination (any dory_tensor_fill_uniform of it does) drives dA, cw and da by those first values -- the caller's, not
    the azrow kept from the forward."""
    before = _primed_snapshot(da, nb, lazy)
    for order in ORDERS:
        ctx, g, v, what = _after_action(da, action, nb, lazy, "apply_edge backward", order, before, vary_az=True)
        cp = np.asarray(g["colPtr"], np.int64)
        first = gr.first_edge(cp, v["az"], np.float32(0))
        assert not _bits(v["az"], gr.expand_rows(cp, first)), what       # the premise: it does vary
        _check_edge_backward(ctx, g, v, gr.expand_rows(cp, first), what)
        ctx.close()


@pytest.mark.parametrize("lazy", [0, 1], ids=["eager", "lazy"])
@pytest.mark.parametrize("nb", [0, 8], ids=["k1", "blocked"])
def test_new_attention_weights_without_an_edge_pass_keep_the_scores(da, nb, lazy):
    """pinned: dory_weight_set("a_i") does not touch az / A / dA or what is kept of them -- the scores are those of the last
    edge pass until the next one, and the aggregations go on using them (the Engine sets weights between epochs only)"""
    ctx, g = _cache_ctx(da, nb, lazy)
    before = _visible(ctx)
    ah, aTg = ctx.download(0, "ah"), ctx.download(0, "aTg")
    ctx.weight_set(0, "a_i", -3.0 * before["a"])
    ctx.aggregate(1, FWD)
    ctx.aggregate(1, BWD)
    v = _visible(ctx)
    for nm in ("az", "A", "dA"):
        assert _bits(v[nm], before[nm]), (nm, nb, lazy)
    assert _bits(ctx.download(0, "ah"), ah) and _bits(ctx.download(0, "aTg"), aTg), (nb, lazy)
    ctx.apply_edge(1, FWD)          # the next edge pass takes the new weights
    fw = gr.edge_forward(g["colPtr"], v["z"], -3.0 * before["a"].astype(np.float64))
    _ratio(("a_i", nb, lazy, "az after the next edge pass"), ctx.download(0, "az").ravel(), fw["az"], fw["b_az"])
    ctx.close()
