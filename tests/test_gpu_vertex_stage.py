"""The vertex stage, kernel by kernel, against float64 numpy (tests/vertex_stage_ref.py): K2 (csrc/gemm.hip: NN with the tanh
epilogue, NT, TN split-K with its second-stage sum), tanh', K4 with the maskout quirk and the validation statistics
(csrc/elementwise.hip) -- driven through dory_apply_vertex on an edgeless graph, so that (V, d_l, d_{l+1}) sets M, N, K of
every product.

Every GEMM case runs with small-integer inputs (every partial sum is exactly representable: the result has to be the integer
product bit for bit, whatever the tile, split or MFMA order) and with random real inputs (the project's parity criteria
against the float64 product); operand padding is NaN before every call, every call is repeated and has to return the same
bits, and an NN product of equal rows has to have equal rows."""
import glob
import os

import numpy as np
import pytest

import vertex_stage_ref as vs

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _edgeless(V):
    """V vertices, no edges (the loader drops self edges): the vertex stage does not look at the graph"""
    import partition_oracle as po
    ids = np.arange(V)
    return po.preprocess(ids, ids, np.zeros(V, np.int64), 0, 1)


def _poison(ctx, layer, names):
    from helpers import _poison_padding
    return sum(_poison_padding(ctx, layer, n) for n in names)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a).view(np.uint32), np.asarray(b).view(np.uint32))


def _check_tanh_of(h, z64, what):
    """test_tanh_matches_libm's bar: 1e-6 relative to libm on the same z, exact zeros stay zero, |h| <= 1"""
    h = h.astype(np.float64)
    ref = np.tanh(z64)
    nz = ref != 0
    if nz.any():
        assert (np.abs(h - ref)[nz] / np.abs(ref[nz])).max() < 1e-6, what
    assert np.array_equal(h[~nz], ref[~nz]) and np.abs(h).max(initial=0.0) <= 1.0, what


def test_case_list_covers_the_plan():
    """the premise: by the mirror of pick_splits / launch_bn (vertex_stage_ref.gemm_plan; its constants are checked against
    gemm.hip by test_vertex_stage_reference.py) every class of the plan occurs in every form that can reach it"""
    got = vs.covered_classes()
    for form, need in vs.REQUIRED_CLASSES.items():
        assert not [c for c in need if c not in got[form]], (form, [c for c in need if c not in got[form]])
    # the tanh epilogue in the kernel (no split) and in the split-K reduce (split)
    nn = [vs.gemm_plan(*vs.gemm_forms(*c)["NN"])["S"] for c in vs.GEMM_CASES]
    assert 1 in nn and max(nn) > 1
    for V, din, dout in vs.GEMM_CASES:
        assert V * max(din, dout) <= 1.5e8 and max(V, din, dout) * vs.INT_MAX ** 2 < 2 ** 24


def _hidden_layer(da, V, din, dout, exact):
    """forward (NN + tanh) and backward (tanh', TN, NT) of a hidden layer din -> dout at layer 1"""
    from helpers import assert_parity, make_ctx
    what = (V, din, dout, "exact" if exact else "real", "hidden")
    ah, W, aTg = vs.gemm_inputs(V, din, dout, exact)
    ctx = make_ctx(da, _edgeless(V), [8, din, dout, 2], V)
    ctx.weight_set(1, "w", W)

    # equal rows in, equal rows out: a lane or tile mapping fault shows even where it rounds like the reference
    ctx.upload(1, "ah", np.broadcast_to(ah[:1], ah.shape))
    _poison(ctx, 1, ["ah"])
    ctx.apply_vertex(1, da.FORWARD)
    for name in ("z", "h"):
        t = ctx.download(1, name).view(np.uint32)
        assert (t == t[:1]).all(), what + (name, "rows of equal inputs differ")

    ctx.upload(1, "ah", ah)
    assert _poison(ctx, 1, ["ah"]) > 0 or din % 32 == 0
    ctx.apply_vertex(1, da.FORWARD)
    z, h = ctx.download(1, "z"), ctx.download(1, "h")
    z64 = vs.mm64(ah, W)
    if exact:
        assert np.array_equal(z, z64), what + ("z", int((z != z64).sum()), np.argwhere(z != z64)[:8].tolist())
        _check_tanh_of(h, z64, what + ("h",))
    else:
        assert_parity(z, z64, what + ("z",))
        assert_parity(h, np.tanh(z64), what + ("h",))
        _check_tanh_of(h, z.astype(np.float64), what + ("h of the GPU's z",))
    _poison(ctx, 1, ["ah"])
    ctx.apply_vertex(1, da.FORWARD)
    assert _same_bits(ctx.download(1, "z"), z) and _same_bits(ctx.download(1, "h"), h), what + ("forward twice",)

    if exact:      # z = 0: tanh' = 1 and g = aTg exactly, so dW and grad are integer products too
        ctx.upload(1, "z", np.zeros((V, dout), np.float32))
        g64 = aTg.astype(np.float64)
    else:
        g64 = vs.tanh_backward64(aTg, z)     # K3 reads the z the GPU holds
    ctx.upload(1, "aTg", aTg)
    out = []
    for rep in range(2):
        _poison(ctx, 1, ["ah", "aTg", "g", "z"])
        ctx.apply_vertex(1, da.BACKWARD)
        out.append((ctx.download(1, "g"), ctx.weight_grad_get(1), ctx.download(1, "grad")))
    g, dW, grad = out[0]
    dW64, grad64 = vs.mm64(ah, g, ta=True), vs.mm64(g, W, tb=True)     # of the g the products read (compared with g64 below)
    if exact:
        assert np.array_equal(g, g64), what + ("g",)
        assert np.array_equal(dW, dW64), what + ("dW", int((dW != dW64).sum()), np.argwhere(dW != dW64)[:8].tolist())
        assert np.array_equal(grad, grad64), what + ("grad", int((grad != grad64).sum()), np.argwhere(grad != grad64)[:8].tolist())
    else:
        assert_parity(g, g64, what + ("g",))
        assert np.isfinite(dW).all() and np.isfinite(grad).all(), what
        assert_parity(dW, dW64, what + ("dW",))
        assert_parity(grad, grad64, what + ("grad",))
    for a, b, name in zip(out[0], out[1], ("g", "dW", "grad")):
        assert _same_bits(a, b), what + (name, "backward twice")
    ctx.close()


def _last_layer(da, V, din, C, exact):
    """forward of the last layer din -> C at layer 1: NN logits (no epilogue), K4, the statistics, NT, TN"""
    from helpers import assert_parity, make_ctx, rel_err, rowsum_err
    what = (V, din, C, "exact" if exact else "real", "last")
    ah, W, _ = vs.gemm_inputs(V, din, C, exact, seed=1)
    labels = np.random.default_rng([V, din, C]).integers(0, C, V).astype(np.uint32)
    lab = vs.onehot(labels, C)
    globalV = 2 * V + 3
    ctx = make_ctx(da, _edgeless(V), [8, din, C], globalV)
    ctx.weight_set(1, "w", W)
    ctx.labels_upload(labels)
    ctx.upload(1, "ah", ah)
    out = []
    for rep in range(2):
        _poison(ctx, 1, ["ah", "z", "g", "lab"])
        ctx.apply_vertex(1, da.FORWARD)
        out.append((ctx.download(1, "z"), ctx.download(1, "g"), ctx.download(1, "grad"), ctx.weight_grad_get(1),
                    np.array(ctx.train_stat(), np.float32)))
    z, g, grad, dW, stat = out[0]
    z64 = vs.mm64(ah, W)
    if exact:
        assert np.array_equal(z, z64), what + ("z", int((z != z64).sum()), np.argwhere(z != z64)[:8].tolist())
    else:
        assert_parity(z, z64, what + ("z",))
    g64 = vs.loss_grad64(z, lab, globalV)      # K4 reads the z the GPU holds
    assert np.isfinite(g).all() and np.isfinite(grad).all() and np.isfinite(dW).all(), what
    if exact:
        # integer logits saturate the softmax: where the label sits on a probability near 1, g is what fp32's p leaves of
        # p - 1 -- cancellation, nothing the element's own size can bound.  The format bounds it instead: K4 makes p of one
        # expf, ceil(C / lanes) + log2(lanes) additions and one division (a few ulp each; 6 allowed for the three calls and the
        # division by the denominator), so |p_fp32 - p| <= k eps p <= k eps, and g = (p - lab) / denom
        lanes = vs.softmax_lanes_per_row(C)
        k = -(-C // lanes) + int(np.log2(lanes)) + 6
        denom = np.float64(np.float32(globalV * 0.66))
        assert np.abs(g * denom - g64 * denom).max(initial=0.0) <= k * np.finfo(np.float32).eps, what + ("g", k)
        assert rel_err(g, g64) < 1e-4 and rowsum_err(g, g64) <= 1.0, what + ("g", rel_err(g, g64), rowsum_err(g, g64))
    else:
        assert_parity(g, g64, what + ("g",))
    # NT and TN against the float64 products of the g they read (checked above): what cancellation left in a row of g is that
    # row's whole content, and no business of the GEMM
    assert_parity(grad, vs.mm64(g, W, tb=True), what + ("grad",))
    assert_parity(dW, vs.mm64(ah, g, ta=True), what + ("dW",))
    acc, loss, rows = vs.train_stat64(z, lab)
    assert int(stat[2]) == rows and float(stat[0]) == acc, what + ("acc", stat.tolist(), acc, rows)
    if not exact:   # (integer logits spread over hundreds: float64's log p is finite where fp32's p is 0 -- the loss cases below)
        assert abs(float(stat[1]) - loss) <= 1e-3 * max(1.0, abs(loss)), what + ("loss", float(stat[1]), loss)
    for a, b, name in zip(out[0], out[1], ("z", "g", "grad", "dW", "stat")):
        assert _same_bits(a, b), what + (name, "forward twice")
    ctx.close()


@pytest.mark.parametrize("mode", ["exact", "real"])
@pytest.mark.parametrize("V,din,dout", vs.GEMM_CASES, ids=[f"V{v}-{a}-{b}" for v, a, b in vs.GEMM_CASES])
def test_gemm_forms(da, V, din, dout, mode):
    """NN / NT / TN of one (V, d_in, d_out) -- as a hidden layer (tanh epilogue) and as the last one (loss in between)"""
    _hidden_layer(da, V, din, dout, mode == "exact")
    _last_layer(da, V, din, dout, mode == "exact")


def test_width_one_layer_is_refused(da):
    """a tensor of one column keeps ld = 1 (per-edge and per-vertex vectors); K2's 16-byte DMA pieces and K3's 16-byte lanes
    need rows that start on 16-byte boundaries, so a layer of width 1 is an error in every stage, forward and backward --
    N = 1 (and M = 1 in TN) of the GEMM are out of reach, and nothing is launched on such rows"""
    from helpers import make_ctx
    V = 40
    for dims, layer in (([8, 1, 4, 2], 1), ([8, 4, 1, 2], 1), ([8, 4, 1], 1)):
        ctx = make_ctx(da, _edgeless(V), dims, V)
        ctx.labels_upload(np.zeros(V, np.uint32))
        with pytest.raises(da.DoryError):
            ctx.apply_vertex(layer, da.FORWARD)
        if len(dims) == 4:
            mark = np.full((V, dims[2]), 5.0, np.float32)
            ctx.upload(layer, "g", mark)
            with pytest.raises(da.DoryError):
                ctx.apply_vertex(layer, da.BACKWARD)
            if dims[2] == 1:      # K3 comes first in that stage: it must not have touched one-column rows either
                assert np.array_equal(ctx.download(layer, "g"), mark)
        ctx.close()


def test_empty_partition_gives_zero_weight_gradient(da):
    """a rank without vertices (tests/golden/parts_toy40_p3_empty): TN with K = 0 is the memset branch -- dW is exactly zero,
    also where an earlier product left something else there, and the statistics are zero"""
    import partition_oracle as po
    from helpers import make_ctx
    d = os.path.join(ROOT, "tests", "golden", "parts_toy40_p3_empty")
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    gs = [po.parse_graph_bin(open(b, "rb").read()) for b in bins]
    empty = [r for r, g in enumerate(gs) if g["localVtxCnt"] == 0]
    assert empty                                             # the premise
    dims = [8, 200, 65, 7]
    for r in empty:
        g = gs[r]
        ctx = make_ctx(da, g, dims, g["globalVtxCnt"], node_id=r, num_nodes=len(gs))
        ctx.labels_upload(np.zeros(0, np.uint32))
        for l in range(3):
            ctx.weight_set(l, "w", np.ones((dims[l], dims[l + 1]), np.float32))
            ctx.weight_grad_set(l, np.full((dims[l], dims[l + 1]), 7.0, np.float32))
        ctx.apply_vertex(1, da.FORWARD)
        ctx.apply_vertex(2, da.FORWARD)
        ctx.apply_vertex(1, da.BACKWARD)
        for l in (1, 2):
            dW = ctx.weight_grad_get(l)
            assert not dW.any() and not np.signbit(dW).any(), (r, l)
        assert ctx.train_stat() == (0.0, 0.0, 0)
        ctx.close()


# ---- K4 and the statistics with logits under the test's control: d_{L-1} = C, W = I, so z = ah exactly ---------------------------
def test_loss_case_list_covers_the_dispatch():
    """the premise of the loss cases: every class and row count of the list occurs, every lanes-per-row and rows-per-block
    value is reached, a case has no validation row, one more than 256 blocks of them, one a window inside one block; masked
    ranges end in the middle of a row, within one row and across several"""
    cases = vs.LOSS_CASES
    for C in vs.LOSS_CLASS_COUNTS:
        assert 2 <= sum(1 for c, n in cases if c == C) <= 3, C
    for N in vs.LOSS_ROW_COUNTS:
        assert sum(1 for c, n in cases if n == N) >= 3, N
    assert {vs.softmax_lanes_per_row(c) for c, n in cases} == {8, 16, 32, 64}
    assert any(vs.softmax_lanes_per_row(c) == 16 and c > 32 for c, n in cases)
    assert {vs.stat_rows_per_block(c) for c, n in cases} == {64, 32, 16, 8, 4, 2, 1}
    val = lambda n: vs.windows(n)[1] - vs.windows(n)[0]
    assert any(val(n) == 0 for c, n in cases) and any(val(n) == 1 for c, n in cases)
    assert any(0 < val(n) < vs.stat_rows_per_block(c) for c, n in cases)
    assert any(-(-val(n) // vs.stat_rows_per_block(c)) > 256 for c, n in cases)
    tail = lambda n: n - vs.windows(n)[0]
    assert any(tail(n) % c and tail(n) > 2 * c for c, n in cases)      # ends mid-row after several whole rows
    assert any(tail(n) % c and tail(n) < c for c, n in cases)          # ends inside its first row


def _loss_case(da, C, N, regime, globalV=None):
    from helpers import make_ctx
    what = (C, N, regime)
    z, labels = vs.loss_inputs(C, N, regime)
    lab = vs.onehot(labels, C)
    globalV = globalV or 3 * N + 1
    ctx = make_ctx(da, _edgeless(N), [8, C, C], globalV)
    ctx.weight_set(1, "w", np.eye(C, dtype=np.float32))
    ctx.labels_upload(labels)
    ctx.upload(1, "ah", z)
    _poison(ctx, 1, ["ah", "z", "g", "lab"])
    ctx.apply_vertex(1, da.FORWARD)
    assert np.array_equal(ctx.download(1, "z"), z), what + ("z = ah I",)
    g, stat = ctx.download(1, "g"), ctx.train_stat()
    ctx.close()
    return z, lab, globalV, g, stat


@pytest.mark.parametrize("C,N", vs.LOSS_CASES, ids=[f"C{c}-N{n}" for c, n in vs.LOSS_CASES])
def test_loss_and_statistics(da, C, N):
    """K4's g element for element (the masked flat range included, wherever it ends) and the validation statistics, the five
    logit regimes taking turns row by row"""
    from helpers import assert_parity
    z, lab, globalV, g, stat = _loss_case(da, C, N, "mixed")
    assert np.isfinite(g).all()
    assert_parity(g, vs.loss_grad64(z, lab, globalV), (C, N, "g"))
    stt = vs.windows(N)[0]
    m0, m1 = stt * C, stt * C + (N - stt)
    assert not g.reshape(-1)[m0:m1].any(), (C, N, "masked range: p := label, so g = 0")
    acc, loss, rows = vs.train_stat64(z, lab)
    assert stat[2] == rows and stat[0] == acc, (C, N, "acc", stat, acc, rows)
    assert abs(stat[1] - loss) <= 1e-3 * max(1.0, abs(loss)), (C, N, "loss", stat[1], loss)


@pytest.mark.parametrize("regime", vs.REGIMES)
@pytest.mark.parametrize("C,N", [(8, 100), (41, 1000), (96, 1000), (1000, 100)], ids=lambda v: str(v))
def test_loss_regimes(da, C, N, regime):
    """one logit regime at a time, so that a failure reads as a regime: ordinary rows, rows of equal logits, ties for the
    maximum (the first index wins the accuracy count), one class 60 above the rest, a common offset of 1e4"""
    from helpers import assert_parity
    z, lab, globalV, g, stat = _loss_case(da, C, N, regime)
    if regime == "ties":
        top = z == z.max(axis=1, keepdims=True)
        assert (top.sum(axis=1) > 1).mean() > 0.5               # the premise
    assert_parity(g, vs.loss_grad64(z, lab, globalV), (C, N, regime, "g"))
    acc, loss, rows = vs.train_stat64(z, lab)
    assert rows >= 10 and stat[2] == rows and stat[0] == acc, (C, N, regime, "acc", stat, acc)
    assert abs(stat[1] - loss) <= 1e-3 * max(1.0, abs(loss)), (C, N, regime, "loss", stat[1], loss)


@pytest.mark.parametrize("labels_hit", [True, False], ids=["label_is_top", "label_is_other"])
@pytest.mark.parametrize("C", [41, 96])
def test_loss_spread_200_vs_c_oracle(da, C, labels_hit):
    """one class 200 above the rest: every other probability underflows to 0 in fp32, and -log(0) is what the reference does
    with a validation row whose label is one of them -- compared with the C oracle (fp32 like the reference), not with float64"""
    import orc
    from helpers import assert_parity, make_ctx
    N = 1000
    rng = np.random.default_rng(C)
    z = rng.uniform(-3, 3, (N, C)).astype(np.float32)
    top = rng.integers(0, C, N)
    z[np.arange(N), top] += np.float32(200.0)
    labels = (top if labels_hit else (top + 1 + rng.integers(0, C - 1, N)) % C).astype(np.uint32)
    lab = vs.onehot(labels, C)
    ctx = make_ctx(da, _edgeless(N), [8, C, C], N)
    ctx.weight_set(1, "w", np.eye(C, dtype=np.float32))
    ctx.labels_upload(labels)
    ctx.upload(1, "ah", z)
    ctx.apply_vertex(1, da.FORWARD)
    g, stat = ctx.download(1, "g"), ctx.train_stat()
    ctx.close()
    ref = orc.vtx_forward_last(z, np.eye(C, dtype=np.float32), lab, N)
    assert_parity(g, ref["d"], (C, labels_hit, "g"))
    assert stat[0] == ref["acc"] == (100.0 if labels_hit else 0.0), (stat, ref["acc"])
    if np.isfinite(ref["loss"]):
        assert abs(stat[1] - ref["loss"]) <= 1e-3 * max(1.0, abs(ref["loss"])), (stat, ref["loss"])
    else:
        assert not labels_hit and stat[1] == ref["loss"], (stat, ref["loss"])


@pytest.mark.parametrize("Fout", [41, 128])
def test_tanh_backward_over_the_range(da, Fout):
    """K3 on its own: g = aTg (1 - tanh^2 z) for z from 1e-6 to saturation, at a width that is a multiple of the kernel's
    four-column lanes and one that is not"""
    from helpers import assert_parity, make_ctx
    V = 4096
    z, aTg = vs.tanh_range_inputs(np.random.default_rng(Fout), V, Fout)
    az = np.abs(z)
    assert az.max() > 20 and (az < 1e-3).mean() > 0.001 and ((az > 0.2) & (az < 0.6)).mean() > 0.01    # the premise: all three regimes
    ctx = make_ctx(da, _edgeless(V), [8, 16, Fout, 2], V)
    ctx.upload(1, "z", z)
    ctx.upload(1, "aTg", aTg)
    _poison(ctx, 1, ["z", "aTg", "g", "ah"])
    ctx.apply_vertex(1, da.BACKWARD)
    g = ctx.download(1, "g")
    ctx.close()
    assert np.isfinite(g).all()
    assert_parity(g, vs.tanh_backward64(aTg, z), (Fout, "g"))
