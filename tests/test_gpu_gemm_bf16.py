"""dory_gemm_bf16 (include/dorylus_hip.h; csrc/gemm_bf16.hip): the vertex transforms on v_mfma_f32_32x32x16_bf16, the fp32 operands
rounded to bf16 on their way into LDS, fp32 sums -- driven through dory_apply_vertex on an edgeless graph as
tests/test_gpu_vertex_stage.py drives K2, so that (V, d_in, d_out) sets M, N, K of the three products.

CONTRACT: a product that takes the kernel equals the fp32-accumulated product of its operands rounded to bf16.  On integers in
-4..4 (exact in bf16, every partial sum exact in fp32) that is the integer product bit for bit; on real inputs products of two bf16
values are exact in fp32 and only the additions round: K terms and S splits, one ulp charged per addition (truncation inside the
matrix unit included), so |got - ref| <= (K + S) 2^-23 (|A^| |B^|)[i, j] against the float64 product of the rounded operands --
tighter than the 2^-9 of the operand rounding for every K below ~10^4, so the fp32 kernel on unrounded operands fails it."""
import numpy as np
import pytest

import vertex_stage_ref as vs
from aggregate_ref import bf16_round

pytestmark = pytest.mark.gpu

T = 32   # GEMM_BF16_BK, the k-tile depth of csrc/gemm_bf16.hip
CASES = [(T - 1, T - 1, T - 1), (T, T, T), (T + 1, T + 1, T + 1), (2 * T + 1, 2 * T + 1, 2 * T + 1),   # K around one and two k-tiles
         (127, 127, 63), (128, 128, 64), (129, 129, 65), (130, 64, 128), (130, 65, 129),             # M around 128, N around 64 / 128
         (1, 17, 15), (333, 300, 300),                                                               # one vertex; ragged, multi-tile
         (500, 1000, 64), (500, 64, 1433), (2000, 1433, 16)]                                         # a split product per form
IDS = [f"V{v}-{a}-{b}" for v, a, b in CASES]


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a):
    return np.asarray(a).view(np.uint32)


class Layer:
    """a hidden layer d_in -> d_out at layer 1 of an edgeless graph: forward is NN + tanh, backward tanh', TN, NT"""

    def __init__(self, da, V, din, dout, exact, mode=None):
        from helpers import make_ctx
        from test_gpu_vertex_stage import _edgeless
        self.da, self.ah, self.W, self.aTg = (da,) + vs.gemm_inputs(V, din, dout, exact)
        self.ctx = make_ctx(da, _edgeless(V), [8, din, dout, 2], V)
        self.ctx.weight_set(1, "w", self.W)
        if mode is not None:
            self.ctx.gemm_bf16(mode)

    def run(self, ah=None, z_back=None):
        """(z, h, g, dW, grad) with NaN in the operands' padding; z_back: the z the backward reads instead of the forward's"""
        from helpers import _poison_padding
        c = self.ctx
        c.upload(1, "ah", self.ah if ah is None else ah)
        _poison_padding(c, 1, "ah")
        c.apply_vertex(1, self.da.FORWARD)
        z, h = c.download(1, "z"), c.download(1, "h")
        if z_back is not None:
            c.upload(1, "z", z_back)
        c.upload(1, "aTg", self.aTg)
        for name in ("aTg", "g", "z"):
            _poison_padding(c, 1, name)
        c.apply_vertex(1, self.da.BACKWARD)
        return z, h, c.download(1, "g"), c.weight_grad_get(1), c.download(1, "grad")


@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("V,din,dout", CASES, ids=IDS)
def test_exact_inputs_bit_for_bit(da, V, din, dout, mode):
    from test_gpu_vertex_stage import _check_tanh_of
    L = Layer(da, V, din, dout, True, mode)
    z, h = L.run(ah=np.broadcast_to(L.ah[:1], L.ah.shape))[:2]     # equal rows in, equal rows out: a lane mapping that rounds like
    assert (_bits(z) == _bits(z)[:1]).all() and (_bits(h) == _bits(h)[:1]).all()   # the reference still shows
    z, h, g, dW, grad = L.run(z_back=np.zeros((V, dout), np.float32))              # z = 0: g = aTg exactly
    z64 = vs.mm64(L.ah, L.W)
    assert np.array_equal(z, z64), ("z", int((z != z64).sum()), np.argwhere(z != z64)[:8].tolist())
    _check_tanh_of(h, z64, "h")
    assert np.array_equal(g, L.aTg)
    for name, got, ref in (("dW", dW, vs.mm64(L.ah, g, ta=True)), ("grad", grad, vs.mm64(g, L.W, tb=True))):
        assert np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:8].tolist())
    assert L.ctx.gemm_bf16_stats() == {"bf16_launches": 2 * (mode + 1), "fp32_while_on": 0}    # two runs of NN, (TN,) NT
    L.ctx.close()


def _ratio(got, A, B, ta=False, tb=False):
    """the largest |got - ref| over its bound (K + S) 2^-23 |A^| |B^|, A^ = bf16(A), ref the float64 product of the rounded operands"""
    Ar, Br = bf16_round(A), bf16_round(B)
    ref, mag = vs.mm64(Ar, Br, ta, tb), vs.mm64(np.abs(Ar), np.abs(Br), ta, tb)
    K = A.shape[0] if ta else A.shape[1]
    bound = (K + vs.gemm_plan(ref.shape[0], ref.shape[1], K)["S"]) * 2.0 ** -23 * mag
    err = np.abs(got.astype(np.float64) - ref)
    assert np.isfinite(got).all() and (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


@pytest.mark.parametrize("V,din,dout", CASES + [(40000, 602, 128)], ids=IDS + ["V40000-602-128"])
def test_real_inputs_against_the_product_of_the_rounded_operands(da, V, din, dout):
    from test_gpu_vertex_stage import _check_tanh_of
    L = Layer(da, V, din, dout, False, 2)
    z, h, g, dW, grad = L.run()
    r = {"z": _ratio(z, L.ah, L.W), "dW": _ratio(dW, L.ah, g, ta=True), "grad": _ratio(grad, g, L.W, tb=True)}
    print("largest error over the bound:", (V, din, dout), r)
    assert max(r.values()) <= 1.0, r
    _check_tanh_of(h, z.astype(np.float64), "h of the GPU's z")
    if (V, din, dout) == (333, 300, 300):      # the bound tells the paths apart: the fp32 kernel on unrounded operands misses it
        L.ctx.gemm_bf16(0)
        assert _ratio(L.run()[0], L.ah, L.W) > 1.0
    L.ctx.close()


@pytest.mark.parametrize("V,din,dout", [(333, 300, 300), (500, 64, 1433)], ids=["nosplit", "split"])
def test_the_switch_moves_nothing_else(da, V, din, dout):
    plain = Layer(da, V, din, dout, False)
    L = Layer(da, V, din, dout, False)
    zb = vs.gemm_inputs(V, din, dout, False, seed=5)[2]     # the z the backward reads: the same g whatever the forward's mode
    ref = plain.run(z_back=zb)
    assert plain.ctx.gemm_bf16_stats() == {"bf16_launches": 0, "fp32_while_on": 0}
    L.ctx.gemm_bf16(1)
    one = L.run(z_back=zb)
    assert L.ctx.gemm_bf16_stats() == {"bf16_launches": 2, "fp32_while_on": 0}
    assert np.array_equal(_bits(one[2]), _bits(ref[2])) and np.array_equal(_bits(one[3]), _bits(ref[3]))     # g; dW: TN stays fp32
    assert not np.array_equal(one[0], ref[0]) and not np.array_equal(one[4], ref[4])                        # z, grad: rounded operands
    L.ctx.gemm_bf16(2)
    two = L.run(z_back=zb)
    assert L.ctx.gemm_bf16_stats() == {"bf16_launches": 5, "fp32_while_on": 0}
    assert not np.array_equal(two[3], ref[3])
    for a, b in zip(two, L.run(z_back=zb)):                 # two runs, the same bits
        assert np.array_equal(_bits(a), _bits(b))
    for a, b in zip((two[0], two[1], two[4]), (one[0], one[1], one[4])):
        assert np.array_equal(_bits(a), _bits(b))
    L.ctx.gemm_bf16(0)
    for a, b, name in zip(L.run(z_back=zb), ref, ("z", "h", "g", "dW", "grad")):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert L.ctx.gemm_bf16_stats() == {"bf16_launches": 8, "fp32_while_on": 0}
    plain.ctx.close()
    L.ctx.close()


@pytest.mark.parametrize("gnn", ["GAT", "GATMH"])
def test_the_other_models_reach_the_kernel(da, gnn):
    """z = h W of layer 0 (both models' forward transform) on exact inputs with mode 1"""
    from test_gpu_vertex_stage import _edgeless
    V, din, dout = 333, 65, 48
    h, W, _ = vs.gemm_inputs(V, din, dout, True)
    ctx = da.Context(0)
    ctx.configure(getattr(da, gnn), [din, dout, 4], V)
    if gnn == "GATMH":
        ctx.gatmh_heads([1, 1])
    ctx.graph_upload(_edgeless(V))
    ctx.preallocate()
    ctx.gemm_bf16(1)
    ctx.weight_set(0, "w", W)
    ctx.upload(0, "h", h)
    ctx.apply_vertex(0, da.FORWARD)
    assert np.array_equal(ctx.download(0, "z"), vs.mm64(h, W))
    assert ctx.gemm_bf16_stats() == {"bf16_launches": 1, "fp32_while_on": 0}
    ctx.close()


def test_bad_modes_are_refused(da):
    ctx = da.Context(0)
    for bad in (-1, 3, 7):
        with pytest.raises(da.DoryError, match="gemm_bf16: mode %d is none of 0" % bad):
            ctx.gemm_bf16(bad)
    ctx.gemm_bf16(2)     # before configure: legal
    ctx.close()
