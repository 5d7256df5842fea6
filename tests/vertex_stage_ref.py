"""The vertex stage in plain float64 numpy -- GEMM, tanh, tanh', softmax / maskout / loss gradient, validation statistics --
a Python mirror of K2's split-K plan, and the case lists the vertex-stage tests share.

tests/test_gpu_vertex_stage.py compares the HIP kernels with these references; tests/test_vertex_stage_reference.py compares
the references with the committed C oracle and the mirror's constants with csrc/gemm.hip, so that both are verified where
there is no GPU."""
import numpy as np

# ---- the split-K plan of csrc/gemm.hip (pick_splits, launch_bn, launch_gemm) --------------------------------------------
# test_vertex_stage_reference.py reads these constants out of gemm.hip: a retuned plan fails there and points here.
BK = 16                   # k-tile depth
BK_SPLIT = 32             # granularity of the split-K plan
GEMM_BM_WIDE = 128        # rows per tile of the 128-wide shape (N > 64)
GEMM_BM_NARROW = 128      # rows per tile of the 64-wide shape (N <= 64)
NO_SPLIT_TILES = 512      # this many output tiles or more: no split
TARGET_WORKGROUPS = 1024  # tiles * S aims at this
MAX_SPLITS = 512
REDUCE_UNROLL = 8         # splitk_reduce_kernel requests eight partials at a time


def _cdiv(a, b):
    return (a + b - 1) // b


def gemm_plan(M, N, K):
    """what launch_gemm does with an M x N x K product: tile shape, grid, split count (as picked and as launched) and the
    rounded k-length of a split"""
    bn = 128 if N > 64 else 64
    bm = GEMM_BM_WIDE if N > 64 else GEMM_BM_NARROW
    rt, ct = _cdiv(M, bm), _cdiv(N, bn)
    tiles = rt * ct
    p = dict(bm=bm, bn=bn, row_tiles=rt, col_tiles=ct, tiles=tiles, capped=False)
    if K == 0 or tiles == 0:
        p.update(S=0, klen=0)
        return p
    if tiles >= NO_SPLIT_TILES or K < 8 * BK_SPLIT:
        s = 1
    else:
        s = _cdiv(TARGET_WORKGROUPS, tiles)
        s = min(s, _cdiv(K, 4 * BK_SPLIT))
        if s > MAX_SPLITS:
            s, p["capped"] = MAX_SPLITS, True
        s = max(s, 1)
    klen = _cdiv(_cdiv(K, s), BK) * BK
    p.update(S=_cdiv(K, klen), klen=klen)
    return p


def gemm_forms(V, din, dout):
    """the (M, N, K) of the three products a layer din -> dout makes of V vertices"""
    return {"NN": (V, dout, din), "NT": (V, din, dout), "TN": (din, dout, V)}


def plan_classes(M, N, K):
    """the classes of the case list's premise (tests/test_gpu_vertex_stage.py) an M x N x K product falls into"""
    p = gemm_plan(M, N, K)
    S, c = p["S"], set()
    if p["tiles"] >= NO_SPLIT_TILES:
        c.add("nosplit_tiles")
    elif K < 8 * BK_SPLIT:
        c.add("nosplit_shortK")
    if 2 <= S <= 7:
        c.add("S2_7")
    if S >= 8 and S % REDUCE_UNROLL:
        c.add("S8p_ragged_unroll")
    if S >= 8 and S % REDUCE_UNROLL == 0:
        c.add("S_mult8")
    if S == MAX_SPLITS and p["capped"]:
        c.add("S_cap")
    if S > 1 and K % p["klen"]:
        c.add("ragged_last_split")
    c.add("K%16==0" if K % BK == 0 else "K%16!=0")
    if K in (1, 15, 16, 17):
        c.add(f"K={K}")
    if N in (63, 64, 65, 127, 128, 129, 200, 256, 300):
        c.add(f"N={N}")
    if M in (1, 127, 128, 129):
        c.add(f"M={M}")
    if p["row_tiles"] >= 3 and M % p["bm"]:
        c.add("M_tiles_ragged")
    if p["row_tiles"] >= 2 and p["col_tiles"] >= 2 and S > 1:
        c.add("rows_x_cols_x_splits")
    return c


# (V, d_in, d_out): M, N, K of the three forms follow (gemm_forms).  A width of 1 is not in the list: such a tensor keeps
# ld = 1 (ctx.hpp pad_ld), K2 moves 16-byte pieces and refuses it -- test_width_one_layer_is_refused.
GEMM_CASES = [
    (1, 17, 15),                                       # one vertex: M = 1 (NN, NT), K = 1 (TN)
    (15, 15, 15), (16, 16, 16), (17, 17, 17),          # K around one k-tile, in every form
    (127, 127, 63), (128, 128, 64), (129, 129, 65),    # M around one row tile, N around the narrow tile
    (130, 63, 127), (130, 64, 128), (130, 65, 129),    # N around the wide tile (NN, TN) / the narrow one (NT)
    (300, 200, 200), (300, 256, 256), (333, 300, 300),  # several row tiles, a ragged last one, 2-3 column tiles, S = 1..3
    (300, 602, 200), (300, 200, 602),                  # row tiles x column tiles x splits, ragged last split
    (500, 1000, 64), (500, 64, 1000),                  # S = 8 exactly (NN / NT)
    (500, 64, 1433), (2000, 1433, 16),                 # S = 12 (NT / NN), S = 16 (TN)
    (300, 1433, 5505),                                 # 528 output tiles in TN; S = 29 in NT
    (2708, 1433, 16), (2708, 16, 7),                   # Cora as it is
    (30000, 1433, 16), (30000, 16, 7),                 # Cora's widths, moderate V
    (30000, 256, 48), (30000, 48, 51),                 # Friendster
    (40000, 602, 128), (40000, 128, 41),               # Reddit
    (66000, 300, 64), (66000, 64, 64), (66000, 64, 25),  # Amazon; 516 row tiles: no split whatever K
    (73700, 64, 32),                                   # TN: S = 512 after the rounding too, ragged last split
    (250000, 64, 32),                                  # tall and narrow
]

# which class has to occur in which form.  K = 1 and M = 1 in TN / N = 1 anywhere would need a width-1 layer (above); the cap
# needs K >= 65 409, i.e. the vertex count as K; 512 tiles in TN need a 5 505-wide layer (one case has it).
_COMMON = ["nosplit_tiles", "nosplit_shortK", "S2_7", "S8p_ragged_unroll", "S_mult8", "ragged_last_split", "K%16==0", "K%16!=0",
           "K=15", "K=16", "K=17", "N=63", "N=64", "N=65", "N=127", "N=128", "N=129", "N=200", "N=256", "N=300",
           "M=127", "M=128", "M=129", "M_tiles_ragged", "rows_x_cols_x_splits"]
REQUIRED_CLASSES = {"NN": _COMMON + ["M=1"], "NT": _COMMON + ["M=1"], "TN": _COMMON + ["K=1", "S_cap"]}


def covered_classes(cases=None):
    got = {f: set() for f in ("NN", "NT", "TN")}
    for V, din, dout in (GEMM_CASES if cases is None else cases):
        for f, (M, N, K) in gemm_forms(V, din, dout).items():
            got[f] |= plan_classes(M, N, K)
    return got


# ---- inputs ---------------------------------------------------------------------------------------------------------------
INT_MAX = 4   # exact inputs are integers in -4..4: K * 4 * 4 < 2^24 for every K below 1 048 576


def exact_inputs(rng, shape):
    return rng.integers(-INT_MAX, INT_MAX + 1, shape).astype(np.float32)


def gemm_inputs(V, din, dout, exact, seed=0):
    """ah (V x din), W (din x dout), aTg (V x dout)"""
    rng = np.random.default_rng([seed, V, din, dout, int(exact)])
    if exact:
        assert max(V, din, dout) * INT_MAX * INT_MAX < 2 ** 24
        return exact_inputs(rng, (V, din)), exact_inputs(rng, (din, dout)), exact_inputs(rng, (V, dout))
    ah = rng.uniform(-1, 1, (V, din)).astype(np.float32)
    W = (rng.standard_normal((din, dout)) / np.sqrt(din)).astype(np.float32)
    aTg = rng.uniform(-1, 1, (V, dout)).astype(np.float32)
    return ah, W, aTg


# ---- float64 references -------------------------------------------------------------------------------------------------------
def mm64(A, B, ta=False, tb=False, chunk=16384):
    """op(A) op(B) in float64 (exact for the integer inputs: every product and sum is an integer far below 2^53), the long
    dimension walked in chunks so that no float64 copy of a whole operand is made"""
    A, B = np.asarray(A), np.asarray(B)
    if ta:       # A is K x M, B is K x N: the reduction runs over the rows
        out = np.zeros((A.shape[1], B.shape[0] if tb else B.shape[1]), np.float64)
        for i in range(0, A.shape[0], chunk):
            b = B[:, i:i + chunk].T if tb else B[i:i + chunk]
            out += A[i:i + chunk].astype(np.float64).T @ b.astype(np.float64)
        return out
    B64 = (B.T if tb else B).astype(np.float64)
    out = np.empty((A.shape[0], B64.shape[1]), np.float64)
    for i in range(0, A.shape[0], chunk):
        out[i:i + chunk] = A[i:i + chunk].astype(np.float64) @ B64
    return out


def tanh_backward64(aTg, z):
    return np.asarray(aTg, np.float64) * (1.0 - np.tanh(np.asarray(z, np.float64)) ** 2)


def softmax64(z):
    """max-subtracted, the denominator seeded with 1e-20 (csrc/elementwise.hip K4)"""
    z = np.asarray(z, np.float64)
    if z.shape[0] == 0:
        return z.copy()
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return e / (e.sum(axis=1, keepdims=True) + 1e-20)


def windows(N):
    """first training-mask row / first and last validation row, as the stage computes them"""
    stt = int(N * 0.66)
    return stt, stt + int(N * 0.1)


def loss_grad64(z, lab, globalV):
    """g = (p - lab) / float32(globalV * 0.66), where p is the softmax with the flat dense-index range
    [stt*C, stt*C + (N - stt)) overwritten by the labels (the reference's maskout copies N - stt FLOATS, not rows)"""
    z = np.asarray(z, np.float64)
    lab = np.asarray(lab, np.float64)
    N, C = z.shape
    p = softmax64(z)
    stt, _ = windows(N)
    pf, lf = p.reshape(-1), lab.reshape(-1)
    pf[stt * C: stt * C + (N - stt)] = lf[stt * C: stt * C + (N - stt)]
    return (p - lab) / np.float64(np.float32(globalV * 0.66))


def train_stat64(z, lab):
    """(acc, loss, rows) over the validation rows: acc += lab[argmax z] (first maximum), loss -= log p[argmax lab]"""
    z = np.asarray(z, np.float64)
    lab = np.asarray(lab, np.float64)
    stt, end = windows(z.shape[0])
    if end == stt:
        return 0.0, 0.0, 0
    zv, lv = z[stt:end], lab[stt:end]
    p = softmax64(zv)
    r = np.arange(end - stt)
    acc = lv[r, zv.argmax(axis=1)].sum()          # numpy's argmax returns the first maximum
    with np.errstate(divide="ignore"):
        loss = -np.log(p[r, lv.argmax(axis=1)]).sum()
    return float(acc), float(loss), end - stt


# ---- loss cases ---------------------------------------------------------------------------------------------------------------------
# (C, N): every class count at a dispatch edge of launch_softmax_rows / stat_rows_per_block with two or three row counts, every
# row count that moves the windows with three or more class counts; the last two reach two rows and one row per block, the first
# of them with more than 256 blocks of validation rows, so that train_stat_final_kernel loops.
LOSS_CASES = [
    (2, 1), (2, 11), (2, 1000), (8, 2), (8, 64), (8, 6401), (9, 9), (9, 65), (16, 10), (16, 100), (17, 11), (17, 1000),
    (32, 63), (32, 6401), (33, 64), (33, 2), (41, 65), (41, 1000), (48, 100), (48, 1), (49, 1000), (49, 9), (64, 6401), (64, 10),
    (65, 1), (65, 63), (95, 2), (95, 100), (96, 9), (96, 1000), (172, 10), (172, 64), (191, 11), (191, 6401), (192, 63),
    (192, 100), (383, 64), (383, 11), (384, 65), (384, 1000), (1000, 100), (1000, 6401), (1000, 9),
    (2000, 6401), (3100, 100),
]
LOSS_CLASS_COUNTS = [2, 8, 9, 16, 17, 32, 33, 41, 48, 49, 64, 65, 95, 96, 172, 191, 192, 383, 384, 1000]
LOSS_ROW_COUNTS = [1, 2, 9, 10, 11, 63, 64, 65, 100, 1000, 6401]
REGIMES = ["uniform", "all_equal", "ties", "dominant60", "offset1e4"]


def stat_rows_per_block(C):
    """csrc/elementwise.hip stat_rows_per_block: the rows of a block's two LDS images have to fit 48 KB"""
    rb = 64
    while rb > 1 and 2 * rb * (C + 1) * 4 > 48 * 1024:
        rb >>= 1
    return rb


def softmax_lanes_per_row(C):
    """csrc/elementwise.hip launch_softmax_rows"""
    return 8 if C <= 8 else 16 if C <= 16 else 32 if C <= 32 else 16 if C <= 48 else 64


def regime_rows(rng, regime, n, C):
    """n rows of logits (fp32) of one regime; the spread of a row stays below 80, so that every float64 probability is a
    normal fp32 number"""
    z = rng.uniform(-3, 3, (n, C)).astype(np.float32)
    if regime == "all_equal":
        z[:] = rng.uniform(-3, 3, (n, 1)).astype(np.float32)
    elif regime == "ties" and C > 1:       # the maximum sits at two or three columns: the first has to win
        top = z.max(axis=1) + np.float32(0.5)
        for k in range(min(3, C)):
            z[np.arange(n), rng.integers(0, C, n)] = top
    elif regime == "dominant60":
        z[np.arange(n), rng.integers(0, C, n)] += np.float32(60.0)
    elif regime == "offset1e4":
        z += np.float32(1e4)
    return z


def loss_inputs(C, N, regime="mixed", seed=0):
    """logits (N x C, fp32) and labels (N, u32).  "mixed": the regimes take turns row by row, so that every window of five
    rows holds all of them; in the ties / dominant rows the label is the first / the raised column every other time"""
    rng = np.random.default_rng([seed, C, N, len(regime)])
    regs = REGIMES if regime == "mixed" else [regime]
    z = np.empty((N, C), np.float32)
    for i, rg in enumerate(regs):
        rows = np.arange(i, N, len(regs))
        z[rows] = regime_rows(rng, rg, rows.size, C)
    labels = rng.integers(0, C, N).astype(np.uint32)
    hit = rng.random(N) < 0.5
    labels[hit] = z[hit].argmax(axis=1).astype(np.uint32)
    return z, labels


def onehot(labels, C):
    return np.eye(C, dtype=np.float32)[np.asarray(labels, np.int64)]


def tanh_range_inputs(rng, V, F):
    """z from 1e-6 to saturation, the magnitudes of test_tanh_matches_libm (10^U(-6, 1.6)) drawn per ELEMENT: every row
    then holds small |z| (derivative ~ 1) next to saturated ones (derivative ~ 1e-30), and the row-scaled absolute term of
    assert_parity covers what 1 - t*t loses to cancellation near |t| = 1 (an fp32 tanh within 1e-6 of libm's leaves
    1 - t^2 an absolute error of 2e-6 at the most -- a fifth of that term in rows like these, whose largest entry is near 1)"""
    z = (rng.uniform(-1, 1, (V, F)) * 10.0 ** rng.uniform(-6, 1.6, (V, F))).astype(np.float32)
    aTg = rng.uniform(-1, 1, (V, F)).astype(np.float32)
    return z, aTg
