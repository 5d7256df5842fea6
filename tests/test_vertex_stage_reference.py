"""The float64 numpy references of the vertex stage (tests/vertex_stage_ref.py) against the committed C oracle, and the Python
mirror of K2's split-K plan against the constants in csrc/gemm.hip -- what tests/test_gpu_vertex_stage.py relies on, checked
where there is no GPU."""
import os
import re

import numpy as np
import pytest

import vertex_stage_ref as vs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the part of the GEMM case list the fp32 triple loop of the oracle walks in seconds
SMALL_GEMM_CASES = [c for c in vs.GEMM_CASES if c[0] * c[1] * c[2] <= 3.5e8]
SMALL_LOSS_CASES = [(2, 11), (8, 64), (9, 9), (17, 1000), (41, 1000), (48, 1), (49, 1000), (64, 10), (65, 63), (96, 1000), (192, 100),
                    (384, 65), (1000, 100)]


def test_subsets_are_parts_of_the_case_lists():
    assert len(SMALL_GEMM_CASES) >= 20 and set(SMALL_LOSS_CASES) <= set(vs.LOSS_CASES)
    got = vs.covered_classes(SMALL_GEMM_CASES)
    for form in ("NN", "NT", "TN"):      # split and unsplit plans, ragged splits and k-tiles are all in the subset
        assert {"nosplit_shortK", "S2_7", "S_mult8", "ragged_last_split", "K%16!=0", "rows_x_cols_x_splits"} <= got[form], form


def test_plan_mirror_matches_gemm_hip():
    """the constants of vertex_stage_ref.gemm_plan as csrc/gemm.hip states them; if this fails the plan was retuned: update
    the mirror (and look at what the GEMM case list of the GPU test still covers -- test_case_list_covers_the_plan)"""
    src = open(os.path.join(ROOT, "dorylus_amd", "csrc", "gemm.hip")).read()

    def one(pattern):
        m = re.findall(pattern, src)
        assert len(m) == 1, (pattern, m)
        return int(m[0])

    assert one(r"constexpr int BK_SPLIT = (\d+);") == vs.BK_SPLIT
    assert one(r"#define GEMM_BM_WIDE (\d+)") == vs.GEMM_BM_WIDE
    assert one(r"#define GEMM_BM_NARROW (\d+)") == vs.GEMM_BM_NARROW
    assert one(r"if \(tiles >= (\d+) \|\| K < 8 \* BK_SPLIT\) return 1;") == vs.NO_SPLIT_TILES
    assert one(r"uint32_t s = \((\d+) \+ tiles - 1\) / tiles;") == vs.TARGET_WORKGROUPS
    assert one(r"const uint32_t maxs = \(K \+ (\d+) \* BK_SPLIT - 1\) / \(\d+ \* BK_SPLIT\);") == 4
    assert one(r"if \(s > (\d+)\) s = \d+;") == vs.MAX_SPLITS and one(r"if \(s > \d+\) s = (\d+);") == vs.MAX_SPLITS
    assert one(r"for \(; z \+ (\d+) <= S; z \+= \d+\)") == vs.REDUCE_UNROLL
    # launch_gemm: the wide shape above 64 columns, 16-deep k-tiles in both; launch_bn: klen rounded up to whole k-tiles
    assert re.search(r"if \(g\.N > 64\) return launch_bn<128, 2, 2, GEMM_BM_WIDE / 64, 2, 16>", src)
    assert re.search(r"return launch_bn<64, 4, 1, GEMM_BM_NARROW / 128, 2, 16>", src)
    assert vs.BK == 16 and "klen = (klen + BK - 1) / BK * BK;" in src and "S = (g.K + klen - 1) / klen;" in src


def test_plan_mirror_by_hand():
    """a few plans worked out by hand from pick_splits / launch_bn"""
    assert vs.gemm_plan(602, 128, 232965)["S"] == 203                    # Reddit's dW: 5 tiles -> 205 splits of 1 137 -> 1 152 rows -> 203 splits
    p = vs.gemm_plan(64, 32, 73700)
    assert (p["S"], p["klen"], p["capped"]) == (512, 144, True)
    assert vs.gemm_plan(66000, 64, 300)["S"] == 1 and vs.gemm_plan(300, 200, 200)["S"] == 1
    assert (vs.gemm_plan(300, 256, 256)["S"], vs.gemm_plan(300, 256, 256)["klen"]) == (2, 128)
    assert vs.gemm_plan(64, 16, 0)["S"] == 0


def test_scratch_clip_is_out_of_reach():
    """abi_context.hip's gemm() caps the split-K scratch at 256 MB and launch_bn then lowers S.  By the plan's own arithmetic
    the cap is never met: below 512 tiles S <= ceil(1024 / tiles), and a tile covers at most bm x 128 padded floats of a
    partial, so S * M * ld stays under (1024 + tiles) * 128 * 128 floats < 101 MB"""
    worst = 0
    for rt in range(1, 512):
        for ct in range(1, 511 // rt + 1):
            M, N = rt * 128, ct * 128 if ct > 1 else 64
            K = 1 << 20
            p = vs.gemm_plan(M, N, K)
            ld = (N + 31) // 32 * 32
            worst = max(worst, p["S"] * M * ld * 4)
    assert 0 < worst < 256 << 20, worst


@pytest.mark.parametrize("V,din,dout", SMALL_GEMM_CASES, ids=[f"V{v}-{a}-{b}" for v, a, b in SMALL_GEMM_CASES])
def test_gemm_reference_vs_oracle(V, din, dout):
    """mm64 == orc.sgemm in the three forms: bit for bit on the integer inputs (the k-ordered fp32 loop is exact there too),
    by the parity criteria on the real ones; then the hidden layer's forward and backward as the oracle sequences them"""
    import orc
    from helpers import assert_parity
    ah, W, aTg = vs.gemm_inputs(V, din, dout, exact=True)
    assert np.array_equal(orc.sgemm(ah, W), vs.mm64(ah, W))
    assert np.array_equal(orc.sgemm(ah, aTg, ta=True), vs.mm64(ah, aTg, ta=True))
    assert np.array_equal(orc.sgemm(aTg, W, tb=True), vs.mm64(aTg, W, tb=True))
    ah, W, aTg = vs.gemm_inputs(V, din, dout, exact=False)
    z, h = orc.vtx_forward_hidden(ah, W)
    z64 = vs.mm64(ah, W)
    assert_parity(z, z64, (V, din, dout, "z"))
    assert_parity(h, np.tanh(z64), (V, din, dout, "h"))
    g, dW, grad = orc.vtx_backward(aTg, z, ah, W, 1)
    g64 = vs.tanh_backward64(aTg, z)
    assert_parity(g, g64, (V, din, dout, "g"))
    assert_parity(dW, vs.mm64(ah, g64, ta=True), (V, din, dout, "dW"))
    assert_parity(grad, vs.mm64(g64, W, tb=True), (V, din, dout, "grad"))


@pytest.mark.parametrize("V,din,C", [c for c in SMALL_GEMM_CASES if c[0] <= 3000][::3], ids=lambda v: str(v))
def test_last_layer_reference_vs_oracle(V, din, C):
    """logits, loss gradient, statistics, NT and TN of the last layer as orc.vtx_forward_last sequences them"""
    import orc
    from helpers import assert_parity
    ah, W, _ = vs.gemm_inputs(V, din, C, exact=False, seed=1)
    labels = np.random.default_rng([V, din, C]).integers(0, C, V).astype(np.uint32)
    lab = vs.onehot(labels, C)
    globalV = 2 * V + 3
    ref = orc.vtx_forward_last(ah, W, lab, globalV)
    z = orc.sgemm(ah, W)
    g64 = vs.loss_grad64(z, lab, globalV)
    assert_parity(ref["d"], g64, (V, din, C, "g"))
    assert_parity(ref["grad"], vs.mm64(g64, W, tb=True), (V, din, C, "grad"))
    assert_parity(ref["dW"], vs.mm64(ah, g64, ta=True), (V, din, C, "dW"))
    acc, loss, rows = vs.train_stat64(z, lab)
    assert ref["acc"] == acc and abs(ref["loss"] - loss) <= 1e-3 * max(1.0, abs(loss)), (ref["acc"], acc, ref["loss"], loss)


@pytest.mark.parametrize("regime", ["mixed"] + vs.REGIMES)
@pytest.mark.parametrize("C,N", SMALL_LOSS_CASES, ids=[f"C{c}-N{n}" for c, n in SMALL_LOSS_CASES])
def test_loss_reference_vs_oracle(C, N, regime):
    """loss_grad64 (the maskout as a flat dense-index range) and train_stat64 == the oracle's softmax / getTrainStat / maskout
    on logits handed over exactly (W = I), every regime"""
    import orc
    from helpers import assert_parity
    z, labels = vs.loss_inputs(C, N, regime)
    lab = vs.onehot(labels, C)
    globalV = 3 * N + 1
    ref = orc.vtx_forward_last(z, np.eye(C, dtype=np.float32), lab, globalV)
    assert (z.max(axis=1) - z.min(axis=1)).max() < 80           # the premise: float64's probabilities are normal fp32 numbers
    g64 = vs.loss_grad64(z, lab, globalV)
    assert_parity(ref["d"], g64, (C, N, regime, "g"))
    stt = vs.windows(N)[0]
    assert not g64.reshape(-1)[stt * C: stt * C + N - stt].any()
    if (N - stt) % C and N - stt > C:                            # the row the masked range ends in: labels first, softmax after
        r, c = divmod(stt * C + N - stt, C)
        assert not g64[r, :c].any() and g64[r, c:].any()
    acc, loss, rows = vs.train_stat64(z, lab)
    assert ref["acc"] == acc, (C, N, regime, ref["acc"], acc)
    assert abs(ref["loss"] - loss) <= 1e-3 * max(1.0, abs(loss)), (C, N, regime, ref["loss"], loss)


def test_first_maximum_wins_the_accuracy_count():
    """two equal maxima, the label on the second: no hit (the reference's argmax keeps the first); on the first: a hit"""
    N, C = 100, 5
    z = np.zeros((N, C), np.float32)
    z[:, 1] = z[:, 3] = 2.0
    assert vs.train_stat64(z, vs.onehot(np.full(N, 3), C))[0] == 0.0
    assert vs.train_stat64(z, vs.onehot(np.full(N, 1), C)) == (10.0, pytest.approx(10 * np.log(2 + 3 * np.exp(-2.0))), 10)


@pytest.mark.parametrize("Fout", [41, 128])
def test_tanh_backward_reference_vs_oracle(Fout):
    import orc
    from helpers import assert_parity
    z, aTg = vs.tanh_range_inputs(np.random.default_rng(Fout), 4096, Fout)
    g = np.empty_like(z)
    orc.lib.orc_tanh_backward(z.size, aTg, z, g)
    assert_parity(g, vs.tanh_backward64(aTg, z), (Fout, "g"))
