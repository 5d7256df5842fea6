"""dory_gemm_bf16_resident (include/dorylus_hip.h; csrc/gemm_bf16_resident.hip): K2b's layer-0 NN and TN products on a resident bf16 copy
of their A operand -- driven through dory_apply_vertex at layer 0 of a GAT-prototype context on an edgeless graph (feats = h@0), so
that (V, d_in, d_out) sets M, K, N: NN is the forward's z = h W, TN the backward's dW = h^T aTg.

CONTRACT: switch on = switch off (K2b), bit for bit.  On integers in -4..4 both are the integer product; on real inputs the result
stays inside K2b's own bound (tests/test_gpu_gemm_bf16.py: (K + S) 2^-23 |A^| |B^| against the float64 product of the rounded
operands).  NaN lies in the padding of h@0 and aTg@0: the copy's k-tail is its own zeros."""
import ctypes as C

import numpy as np
import pytest

import vertex_stage_ref as vs

pytestmark = pytest.mark.gpu

CASES = [(31, 31, 31), (32, 32, 32), (33, 33, 33), (65, 65, 65), (127, 127, 63), (128, 128, 64), (129, 129, 65), (1, 17, 15),
         (333, 300, 300), (500, 64, 1433), (2000, 1433, 16)]
IDS = [f"V{v}-{a}-{b}" for v, a, b in CASES]
STATS0 = {"resident_launches": 0, "conversions": 0, "plain_while_on": 0}


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a):
    return np.asarray(a).view(np.uint32)


class Layer0:
    """layer 0 of a GAT prototype d_in -> d_out on V edgeless vertices, dory_gemm_bf16 at mode 2"""

    def __init__(self, da, V, din, dout, exact, resident):
        from helpers import _poison_padding, make_ctx
        from test_gpu_vertex_stage import _edgeless
        self.da, self.h, self.W, self.aTg = (da,) + vs.gemm_inputs(V, din, dout, exact)
        c = self.ctx = make_ctx(da, _edgeless(V), [din, dout, 2], V, gnn=da.GAT)
        c.gemm_bf16(2)
        c.gemm_bf16_resident(resident)
        c.weight_set(0, "w", self.W)
        c.upload(0, "h", self.h)
        c.upload(0, "aTg", self.aTg)
        for name in ("h", "aTg"):
            _poison_padding(c, 0, name)

    def epoch(self):
        c = self.ctx
        c.apply_vertex(0, self.da.FORWARD)
        c.apply_vertex(0, self.da.BACKWARD)
        return c.download(0, "z"), c.weight_grad_get(0)


@pytest.mark.parametrize("V,din,dout", CASES, ids=IDS)
def test_exact_inputs_against_float64(da, V, din, dout):
    L = Layer0(da, V, din, dout, True, 1)
    for _ in range(2):
        z, dW = L.epoch()
        assert np.array_equal(z, vs.mm64(L.h, L.W)), ("z", np.argwhere(z != vs.mm64(L.h, L.W))[:8].tolist())
        assert np.array_equal(dW, vs.mm64(L.h, L.aTg, ta=True)), ("dW", np.argwhere(dW != vs.mm64(L.h, L.aTg, ta=True))[:8].tolist())
    assert L.ctx.gemm_bf16_resident_stats() == {"resident_launches": 4, "conversions": 1, "plain_while_on": 0}
    L.ctx.close()


@pytest.mark.parametrize("V,din,dout", CASES, ids=IDS)
def test_real_inputs_switch_on_equals_switch_off(da, V, din, dout):
    from test_gpu_gemm_bf16 import _ratio
    off, on = Layer0(da, V, din, dout, False, 0), Layer0(da, V, din, dout, False, 1)
    ref, one, two = off.epoch(), on.epoch(), on.epoch()
    for name, r, a, b in zip(("z", "dW"), ref, one, two):
        assert np.array_equal(_bits(a), _bits(r)) and np.array_equal(_bits(b), _bits(r)), name
    r = {"z": _ratio(one[0], on.h, on.W), "dW": _ratio(one[1], on.h, on.aTg, ta=True)}
    print("largest error over K2b's bound:", (V, din, dout), r)
    assert max(r.values()) <= 1.0, r
    assert off.ctx.gemm_bf16_resident_stats() == STATS0
    assert on.ctx.gemm_bf16_resident_stats() == {"resident_launches": 4, "conversions": 1, "plain_while_on": 0}
    off.ctx.close()
    on.ctx.close()


def test_a_changed_operand_is_converted_again(da):
    from test_gpu_gemm_bf16 import _ratio
    V, din, dout = 129, 129, 65
    L = Layer0(da, V, din, dout, True, 1)
    c, stats = L.ctx, L.ctx.gemm_bf16_resident_stats
    L.epoch()
    assert stats()["conversions"] == 1
    h2 = vs.gemm_inputs(V, din, dout, True, seed=1)[0]           # an upload
    c.upload(0, "h", h2)
    assert np.array_equal(L.epoch()[0], vs.mm64(h2, L.W)) and stats()["conversions"] == 2
    c.fill_uniform(0, "h", 3)                                     # a fill
    assert _ratio(L.epoch()[0], c.download(0, "h"), L.W) <= 1.0 and stats()["conversions"] == 3
    h3 = vs.gemm_inputs(V, din, dout, True, seed=2)[0]           # a raw pointer handed out, and written through
    rows, cols, ld, p = c.info(0, "h")
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy2D.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.c_size_t, C.c_size_t, C.c_int]
    c.sync()
    assert hip.hipMemcpy2D(C.c_void_p(p), ld * 4, h3.ctypes.data_as(C.c_void_p), cols * 4, cols * 4, rows, 1) == 0
    z, dW = L.epoch()
    assert np.array_equal(z, vs.mm64(h3, L.W)) and np.array_equal(dW, vs.mm64(h3, L.aTg, ta=True))
    assert stats() == {"resident_launches": 8, "conversions": 4, "plain_while_on": 0}
    c.gemm_bf16_split(1)                                          # K2c: an eligible operand, run plain and counted
    assert np.array_equal(L.epoch()[0], vs.mm64(h3, L.W))
    assert stats() == {"resident_launches": 8, "conversions": 4, "plain_while_on": 2} and c.gemm_bf16_split_stats() == {"split_launches": 2}
    c.gemm_bf16_split(0)
    c.gemm_bf16(0)                                                # inert without the bf16 kernel
    L.epoch()
    assert stats() == {"resident_launches": 8, "conversions": 4, "plain_while_on": 2}
    c.gemm_bf16(2)
    c.gemm_bf16_resident(0)                                       # off: the copy is freed, K2b runs
    z, dW = L.epoch()
    assert np.array_equal(z, vs.mm64(h3, L.W)) and np.array_equal(dW, vs.mm64(h3, L.aTg, ta=True))
    assert stats() == {"resident_launches": 8, "conversions": 4, "plain_while_on": 2}
    c.gemm_bf16_resident(1)                                       # ... and on again: a new copy
    assert np.array_equal(L.epoch()[0], vs.mm64(h3, L.W)) and stats()["conversions"] == 5
    for bad in (-1, 2):
        with pytest.raises(da.DoryError, match="gemm_bf16_resident: value %d is neither 0 nor 1" % bad):
            c.gemm_bf16_resident(bad)
    c.close()


def test_the_8_head_gat_reaches_it(da):
    from test_gpu_vertex_stage import _edgeless
    V, din, dout = 333, 65, 48
    h, W, dz = vs.gemm_inputs(V, din, dout, True)
    ctx = da.Context(0)
    ctx.configure(da.GATMH, [din, dout, 4], V)
    ctx.gatmh_heads([1, 1])
    ctx.graph_upload(_edgeless(V))
    ctx.preallocate()
    ctx.gemm_bf16(2)
    ctx.gemm_bf16_resident(1)
    ctx.weight_set(0, "w", W)
    ctx.upload(0, "h", h)
    ctx.upload(0, "dz", dz)
    for _ in range(2):
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_vertex(0, da.BACKWARD)
        assert np.array_equal(ctx.download(0, "z"), vs.mm64(h, W)) and np.array_equal(ctx.weight_grad_get(0), vs.mm64(h, dz, ta=True))
    assert ctx.gemm_bf16_resident_stats() == {"resident_launches": 4, "conversions": 1, "plain_while_on": 0}
    ctx.close()


def _gcn_rank0(da, dims, options):
    """rank 0 of the two-partition golden graph as a GCN context with exact layer-0 inputs: (ctx, x, fg, W)"""
    from gat_stage_ref import golden
    from helpers import make_ctx
    g = golden("parts_toy60_p2")[0]
    ctx = make_ctx(da, g, dims, int(g["globalVtxCnt"]), options=options)
    ctx.gemm_bf16(2)
    rng = np.random.default_rng(7)
    N, G = ctx.info(0, "x", ptr=False)[0], ctx.info(0, "fg", ptr=False)[0]
    x, fg, W = (vs.exact_inputs(rng, s) for s in ((N, dims[0]), (G, dims[0]), (dims[0], dims[1])))
    ctx.weight_set(0, "w", W)
    ctx.upload(0, "x", x)
    ctx.upload(0, "fg", fg)
    return ctx, x, fg, W


def test_gcn_transform_first_keeps_x_and_its_ghost_rows(da):
    ctx, x, fg, W = _gcn_rank0(da, [40, 24, 4], {"gcn_transform_first": 1})
    assert ctx.transform_first_active() and fg.shape[0] > 0
    ctx.gemm_bf16_resident(1)
    for _ in range(2):
        ctx.aggregate(0, da.FORWARD)
        assert np.array_equal(ctx.download(0, "xw"), vs.mm64(x, W)) and np.array_equal(ctx.download(0, "fgxw"), vs.mm64(fg, W))
    assert ctx.gemm_bf16_resident_stats() == {"resident_launches": 4, "conversions": 2, "plain_while_on": 0}
    ctx.close()


@pytest.mark.parametrize("cache", [1, 0])
def test_gcn_aggregate_first_keeps_ah0_only_under_the_cache(da, cache):
    from test_gpu_gemm_bf16 import _ratio
    out = {}
    for resident in (0, 1):
        ctx, x, fg, W = _gcn_rank0(da, [40, 24, 4], {"gcn_cache_ah0": cache})
        ctx.gemm_bf16_resident(resident)
        for _ in range(2):
            ctx.aggregate(0, da.FORWARD)
            ctx.apply_vertex(0, da.FORWARD)
        out[resident] = (ctx.download(0, "z"), ctx.download(0, "h"))
        if resident:
            assert _ratio(out[1][0], ctx.download(0, "ah"), W) <= 1.0
            st = ctx.gemm_bf16_resident_stats()
            assert ctx.get_option("gcn_cache_ah0_skips") == cache      # epoch 2 launched no layer-0 aggregation under the cache
            assert st == ({"resident_launches": 2, "conversions": 1, "plain_while_on": 0} if cache else
                          {"resident_launches": 0, "conversions": 0, "plain_while_on": 2}), st
        ctx.close()
    assert np.array_equal(_bits(out[0][0]), _bits(out[1][0])) and np.array_equal(_bits(out[0][1]), _bits(out[1][1]))


@pytest.mark.parametrize("V,din,dout", [(333, 65, 129), (333, 129, 65), (500, 1000, 64)], ids=["128-wide", "64-wide", "split"])
def test_the_tanh_epilogue_and_the_split_reduce_write_h(da, V, din, dout):
    """GCN layer 0 under gcn_cache_ah0 on real inputs: z = ah@0 W and h = tanh(z) leave K2r's store loop (a split launch: the reduce
    kernel), g and dW = ah@0^T g follow in the backward -- all four as with the switch off, h the tanh of the GPU's z"""
    from helpers import random_graph
    from test_gpu_vertex_stage import _check_tanh_of
    assert (vs.gemm_plan(V, dout, din)["S"] > 1) == (din == 1000)
    s, d = random_graph(5, V, 4 * V)
    part = da.Partition.build(s, d, np.zeros(V, np.int32), 0, 1)
    x, W, aTg = vs.gemm_inputs(V, din, dout, False)
    out = {}
    for resident in (0, 1):
        ctx = da.Context(0)
        ctx.configure(da.GCN, [din, dout, 2], V)
        ctx.set_option("gcn_cache_ah0", 1)
        part.upload(ctx)
        ctx.preallocate()
        ctx.gemm_bf16(2)
        ctx.gemm_bf16_resident(resident)
        ctx.weight_set(0, "w", W)
        ctx.upload(0, "x", x)
        ctx.upload(0, "aTg", aTg)
        for _ in range(2):
            ctx.aggregate(0, da.FORWARD)
            ctx.apply_vertex(0, da.FORWARD)
            ctx.apply_vertex(0, da.BACKWARD)
        out[resident] = [ctx.download(0, n) for n in ("z", "h", "g")] + [ctx.weight_grad_get(0)]
        assert ctx.gemm_bf16_resident_stats() == ({"resident_launches": 4, "conversions": 1, "plain_while_on": 0} if resident else STATS0)
        ctx.close()
    for name, a, b in zip(("z", "h", "g", "dW"), out[0], out[1]):
        assert np.array_equal(_bits(a), _bits(b)), name
    _check_tanh_of(out[1][1], out[1][0].astype(np.float64), "h of the GPU's z")
    assert np.abs(out[1][1]).max() > 0.1
