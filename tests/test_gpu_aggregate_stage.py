"""The aggregation kernels -- K1 (row gather), K1b (partial rows per source block), K1s (the gated sweep) and their bf16 forms --
called through the C-ABI and compared with the float64 reference of tests/aggregate_ref.py:

  * exact mode: signed powers of two as edge values and norm, small integers as features.  Every partial sum in every order is
    exact in fp32 (aggregate_ref.exact_ok, asserted per case) and the integers survive the rounding to bf16, so ONE array
    decides every family, every schedule and both row formats bit for bit: a dropped, doubled or mis-paired edge, a wrong
    ghost index or a row nobody wrote is a bit difference.  (Only the sign of a zero depends on the order -- -0 + -0 against
    -0 + +0 -- so zeros are compared as +0.)
  * real mode: the graphs' GCN values and normal features, every element inside the bound an fp32 sum of the row's terms has
    in any order (aggregate_ref.fp32_sum_bound; derived, and checked against the C oracle where there is no GPU).
  * which family ran: the read-only counters spmm_launches_k1s / _k1b / _k1 against the mirror's prediction.

The case list, the mirror and the proof that the cases reach every form are tests/aggregate_ref.py and
tests/test_aggregate_stage_reference.py."""
import glob
import os

import numpy as np
import pytest

import aggregate_ref as ar

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = {"k1s": "spmm_launches_k1s", "k1b": "spmm_launches_k1b", "k1": "spmm_launches_k1"}
WALKED = dict(ar.WALK)


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _tensors(da, direction):
    """(layer, direction, local rows, ghost rows, output) of the three aggregations a two-layer GCN context offers"""
    return {"fwd0": (0, da.FORWARD, (0, "x"), (0, "fg"), (0, "ah")),
            "fwd1": (1, da.FORWARD, (0, "h"), (1, "fg"), (1, "ah")),
            "bwd": (1, da.BACKWARD, (1, "grad"), (0, "bg"), (0, "aTg"))}[direction]


class Held:
    """one context per case and value mode, kept while that case's tests run (the case is the outermost parameter): the
    families and directions of a case share the uploaded graph, its layouts, the gate counters, scratch and partial buffers --
    which is what a training run does with them.  The case's options are set before the graph is uploaded and the tensors
    are allocated: a layout that dory_preallocate found not applicable (an L2-sized graph without a block count) stays so for
    the life of the upload -- a block count set afterwards does not bring it back, the next family runs (the counters show it)"""

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
                    self.data[direction] = (ref32,)
                else:
                    rows = {False: (x, xg), True: (ar.bf16_round(x), ar.bf16_round(xg))}
                    self.data[direction] = {bf: (ar.aggregate(ptr, idx, val, g["norm"], a, b, 1),
                                                 ar.fp32_sum_bound(ptr, idx, val, g["norm"], a, b, 1)) for bf, (a, b) in rows.items()}
        return self.ctx


@pytest.fixture(scope="module")
def held():
    h = Held()
    yield h
    h.close()


def _bits(a):
    return (np.asarray(a, np.float32) + np.float32(0)).view(np.uint32)      # -0 -> +0; NaN stays NaN


def _mirror_applies(ctx):
    """the mirror assumes 8 XCDs of 32 CUs"""
    try:
        import torch
        cus = torch.cuda.get_device_properties(0).multi_processor_count
    except Exception:
        return False
    return ctx.get_option("spmm_xcd_count") == 8 and cus // 8 == ar.CUS_PER_XCD


def _set(ctx, family, setting):
    ctx.set_option("spmm_variant", ar.FAMILIES[family])
    for key, vals in ar.WALK:
        ctx.set_option(key, setting.get(key, vals[0]))


def _aggregate_counted(ctx, da, layer, dirn):
    before = {f: ctx.get_option(k) for f, k in COUNTERS.items()}
    ctx.aggregate(layer, dirn)
    return {f: ctx.get_option(k) - before[f] for f, k in COUNTERS.items()}


def _check_counters(moved, rec, mirror_ok, what):
    assert sorted(moved.values()) == [0, 0, 1], (what, moved)                  # one family, once
    if mirror_ok:
        assert moved[rec["family"]] == 1, (what, "the mirror expected", rec["family"], "ran", moved, rec)


def _walk_exact(ctx, da, family, direction, ref32, record, mirror_ok, what):
    layer, dirn, _, _, out = _tensors(da, direction)
    want = _bits(ref32)
    nan = np.full(ref32.shape, np.nan, np.float32)
    settings = ar.walk_settings(family)
    for i, setting in enumerate(settings):
        _set(ctx, family, setting)
        ctx.upload(out[0], out[1], nan)                                        # a row the kernels never write must show
        moved = _aggregate_counted(ctx, da, layer, dirn)
        got = ctx.download(out[0], out[1])
        rec = record(setting)
        bad = np.nonzero((_bits(got) != want).any(axis=1))[0]
        assert bad.size == 0, (what, setting, rec["family"], "rows that differ", bad.size, bad[:8].tolist(),
                               "got", got[bad[0], :4].tolist(), "want", ref32[bad[0], :4].tolist(), {k: v for k, v in rec.items() if k != "options"})
        _check_counters(moved, rec, mirror_ok, (what, setting))
        if i in (0, len(settings) - 1):                                        # again into the same context: gate counters, scratch, partials
            ctx.aggregate(layer, dirn)
            assert np.array_equal(_bits(ctx.download(out[0], out[1])), want), (what, setting, "second aggregation")
    _set(ctx, family, {})


PARAMS = [pytest.param(c, f, d, id=f"{c[0]}-{f}-{d}") for c in ar.CASES for f in ar.FAMILIES for d in ar.DIRECTIONS]


@pytest.mark.parametrize("case,family,direction", PARAMS)
def test_aggregate_exact(da, held, case, family, direction):
    """bit for bit against the integer reference, over every schedule that must not change a bit (aggregate_ref.walk_settings:
    spmm_blk_force_split, spmm_order, spmm_edge_split, spmm_sweep_pair, spmm_sweep_loader, gcn_bf16_gather), output poisoned
    with NaN before every aggregation, the first and the last setting aggregated twice"""
    cid, gname, F, options = case
    g = ar.graph(gname)
    ctx = held.get(da, (cid, "exact"), g, F, options, True)
    (ref32,) = held.data[direction]
    _walk_exact(ctx, da, family, direction, ref32, lambda s: ar.case_record(case, family, direction, s), _mirror_applies(ctx),
                (cid, family, direction))


@pytest.mark.parametrize("case,family,direction", PARAMS)
def test_aggregate_real(da, held, case, family, direction):
    """GCN's own values and normal features: |got - ref64| <= gamma_(n+2) * (|self x| + sum |val x|) per element, n the row's
    degree; the bf16 runs against the reference on the rounded rows.  The bound is derived (fp32_sum_bound), not measured"""
    cid, gname, F, options = case
    g = ar.graph(gname, "real")
    ctx = held.get(da, (cid, "real"), g, F, options, False)
    layer, dirn, _, _, out = _tensors(da, direction)
    settings = [{}, {"spmm_blk_force_split": 1}] + ([] if family == "k1b" else [{"gcn_bf16_gather": 2}, {"gcn_bf16_gather": 2, "spmm_blk_force_split": 1}])
    nan = np.full((int(g["localVtxCnt"]), F), np.nan, np.float32)
    for setting in settings:
        _set(ctx, family, setting)
        ctx.upload(out[0], out[1], nan)
        ctx.aggregate(layer, dirn)
        got = ctx.download(out[0], out[1]).astype(np.float64)
        ref, bound = held.data[direction][bool(setting.get("gcn_bf16_gather"))]
        err = np.abs(got - ref)
        ok = err <= bound                                                      # (NaN compares false)
        worst = float(np.nanmax(err / np.maximum(bound, 1e-300))) if got.size else 0.0
        print(f"{cid} {family} {direction} {setting}: worst |err| / bound = {worst:.3f}")
        assert ok.all(), (cid, family, direction, setting, "elements outside the bound", int((~ok).sum()), "worst / bound", worst)
    _set(ctx, family, {})


# ---- the partitions the reference's own loader wrote, with their structure and exact values -------------------------------------------
def _golden_partitions(name):
    import partition_oracle as po
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    return [po.parse_graph_bin(open(b, "rb").read()) for b in bins]


GOLDEN = [("parts_toy60_p1", 128, {"spmm_blk_nb": 8}), ("parts_toy60_p2", 128, {"spmm_blk_nb": 8}), ("parts_toy60_p4_hash", 64, {"spmm_blk_nb": 16}),
          ("parts_toy97_p8_und", 41, {"spmm_blk_nb": 8}), ("parts_toy40_p3_empty", 602, {"spmm_blk_nb": 24}), ("parts_toy60_p2", 300, {}),
          ("parts_hub3000_p2", 41, {"spmm_blk_nb": 8}), ("parts_hub3000_p2", 128, {"spmm_blk_nb": 16}), ("parts_hub3000_p2", 602, {})]


@pytest.mark.parametrize("family", list(ar.FAMILIES))
@pytest.mark.parametrize("name,F,options", GOLDEN, ids=[f"{n}-F{F}-nb{o.get('spmm_blk_nb', 0)}" for n, F, o in GOLDEN])
def test_golden_partitions_exact(da, name, F, options, family):
    """tests/golden/parts_*: bytes of graph.<id>.bin as the reference's loader writes them (ghost numbering, edge order, empty
    partitions; parts_hub3000_p2: rows beyond every clamp) with exact values substituted -- every partition, three directions"""
    from helpers import make_ctx
    for r, g0 in enumerate(_golden_partitions(name)):
        g = ar.substitute_exact_values(g0, seed=r)
        N = int(g["localVtxCnt"])
        ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), node_id=r, num_nodes=max(r + 1, 2), options=options)
        mirror_ok = _mirror_applies(ctx)
        for direction in ar.DIRECTIONS:
            ptr, idx, val, ghosts = ar.side(g, direction)
            x, xg = ar.features(g, direction, F, True, seed=r)
            ar.exact_ok(ptr, idx, val, g["norm"], x, xg, 1)
            ref32 = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1).astype(np.float32)
            _, _, xl_name, xg_name, _ = _tensors(da, direction)
            ctx.upload(xl_name[0], xl_name[1], x)
            ctx.upload(xg_name[0], xg_name[1], xg)
            if N == 0:
                continue
            stats = ar.AdjStats(N, ptr, idx)

            def record(setting, direction=direction, ptr=ptr, idx=idx, ghosts=ghosts, stats=stats):
                o = dict(options, spmm_variant=ar.FAMILIES[family], layout_loader=1)
                o.update(setting)
                o["gcn_bf16_gather"] = int(ar.bf16_on(o, direction))
                return ar.dispatch(N, ghosts, F, ptr, idx, o, static_ghosts=direction == "fwd0", stats=stats)

            _walk_exact(ctx, da, family, direction, ref32, record, mirror_ok, (name, r, F, family, direction))
        ctx.close()


# ---- the unit-weight form: the GAT prototype's neighbour sum ------------------------------------------------------------------------
@pytest.mark.parametrize("case", ar.UNIT_CASES, ids=ar.UNIT_CASE_IDS)
def test_unit_weight_neighbour_sum(da, case):
    """integer z / fg_z, apply_edge, aggregate forward on a GAT context: "nsum" is the integer neighbour sum bit for bit (unit
    weights: the adjacency's values are not read), "ah" = z + arow (.) nsum from the downloaded arow within the two roundings
    of a multiply and an add (one, if fused); with gat_reuse_nsum = 0 the aggregation applies the row factor itself and is
    held to the bound of an fp32 sum (test_gat_without_a_layout_takes_k1: the same for a context without a layout)"""
    from helpers import make_ctx
    cid, gname, F, options = case
    g = ar.graph(gname)
    N = int(g["localVtxCnt"])
    ptr, idx, _, ghosts = ar.side(g, "fwd0")
    rng = np.random.default_rng([41, N, F])
    z, fgz = ar.exact_features(rng, N, F), ar.exact_features(rng, ghosts, F)
    ones = np.ones(len(idx), np.float32)
    ar.exact_ok(ptr, idx, ones, None, z, fgz, 0)
    nsum_ref = ar.aggregate(ptr, idx, ones, None, z, fgz, 0)
    for reuse in (1, 0):
        ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), gnn=da.GAT, options=dict(options, gat_reuse_nsum=reuse))
        ctx.weight_set(0, "a_i", (rng.standard_normal((F, 1)) / F).astype(np.float32))
        ctx.upload(0, "z", z)
        ctx.upload(0, "fg_z", fgz)
        ctx.apply_edge(1, da.FORWARD)
        for again in (0, 1):
            ctx.upload(0, "nsum", np.full((N, F), np.nan, np.float32))
            ctx.upload(0, "ah", np.full((N, F), np.nan, np.float32))
            moved = _aggregate_counted(ctx, da, 1, da.FORWARD)
            arow = ctx.download(0, "arow").astype(np.float64)
            ah = ctx.download(0, "ah").astype(np.float64)
            assert np.isfinite(arow).all()
            ref = z.astype(np.float64) + arow * nsum_ref
            mag = np.abs(z) + np.abs(arow * nsum_ref)
            rec = ar.unit_record(case)
            _check_counters(moved, rec, _mirror_applies(ctx), (cid, reuse, again))
            assert rec["family"] in ("k1s", "k1b") and rec["unit"]
            if reuse:
                assert np.array_equal(_bits(ctx.download(0, "nsum")), _bits(nsum_ref.astype(np.float32))), (cid, again)
                assert (np.abs(ah - ref) <= 2 * 2.0 ** -24 * mag).all(), (cid, again)
            else:      # the same layouts, the row factor inside the kernels: out = z + arow * sum
                A = np.repeat(arow.ravel(), np.diff(ptr.astype(np.int64)))
                assert (np.abs(ah - ref) <= ar.fp32_sum_bound(ptr, idx, A, None, z, fgz, 2)).all(), (cid, again)
        ctx.close()


def test_gat_without_a_layout_takes_k1(da):
    """a GAT partition whose source rows fit one L2 has no blocked layout: K1 on the per-edge scores, inside the bound"""
    from helpers import make_ctx
    g = ar.graph("uniform:1025:12000")
    N, F = 1025, 64
    ptr, idx, _, _ = ar.side(g, "fwd0")
    rng = np.random.default_rng(43)
    z = ar.exact_features(rng, N, F)
    ctx = make_ctx(da, g, [F, F, 3], N, gnn=da.GAT)
    ctx.weight_set(0, "a_i", (rng.standard_normal((F, 1)) / F).astype(np.float32))
    ctx.upload(0, "z", z)
    ctx.apply_edge(1, da.FORWARD)
    ctx.upload(0, "ah", np.full((N, F), np.nan, np.float32))
    moved = _aggregate_counted(ctx, da, 1, da.FORWARD)
    # (twice: the attempt at the unit-weight neighbour sum falls through to K1, which gathers with the per-edge values and so
    # cannot give it -- last_spmm_unit stays false -- then the general path runs)
    assert moved["k1s"] == 0 and moved["k1b"] == 0 and moved["k1"] in (1, 2), moved
    A = ctx.download(0, "A").ravel().astype(np.float64)
    ah = ctx.download(0, "ah").astype(np.float64)
    err = np.abs(ah - ar.aggregate(ptr, idx, A, None, z, None, 2))
    assert (err <= ar.fp32_sum_bound(ptr, idx, A, None, z, None, 2)).all()
    ctx.close()


def test_counters_are_read_only_and_start_at_zero(da):
    from helpers import make_ctx
    g = ar.graph("uniform:1025:12000")
    ctx = make_ctx(da, g, [32, 32, 3], 1025)
    assert [ctx.get_option(k) for k in COUNTERS.values()] == [0, 0, 0]
    with pytest.raises(da.DoryError):
        ctx.set_option("spmm_launches_k1", 5)
    ctx.close()
