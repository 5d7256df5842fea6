"""The reference GAT prototype's edge stage and its aggregations in plain float64 numpy, stated the way CPU_comm.cpp /
gat_ops.cpp (and oracle/dory_oracle.c after them) state them -- per EDGE, with the E x F intermediate and the F x F matrix
built -- so that they share no shortcut with the kernels (one value per destination, r = grad^T cw, da = z^T (z r), one
neighbour sum for two aggregations).  Every reference returns, next to its value, a per-element bound on what a correct fp32
implementation may differ by, derived from the float64 magnitudes of the same inputs (rules below): a test reports
max |got - ref| / bound, and a sum that cancels is judged by what was summed, not by what is left.

Also here: a Python mirror of launch_colsum_w's plan (csrc/elementwise.hip), the case lists with the classes they are there
for and their graphs, the two input families, and a float64 epoch of the prototype over partitions.

tests/test_gpu_gat_stage.py compares the HIP kernels with these references; tests/test_gat_stage_reference.py compares the
references with the committed C oracle, the mirror's constants with the source text and the case lists with their classes,
where there is no GPU.

The prototype's edge scores depend on the destination only: "az", "A" and "dA" hold one value per destination vertex, and the
library keeps that value ("azrow", "arow", "drow").  A caller's own "az" is read at the first in-edge of every destination
(edge_backward_gat_kernel); the cases here upload an "az" that is constant over a destination's edges, as every "az" the
stage computes is, and the references stay the per-edge definition.  The first-edge reading is pinned in one named GPU test,
test_callers_az_is_read_at_the_first_in_edge.

The bounds of dA, y and da are a shade wider than the bare rule: dA on the branch of slope 0.01 counts one more rounding per
term (grad * 0.01f is rounded before it is multiplied), and y and da are bounded with |r| + b_r and |y| + b_y in place of |r|
and |y| (the sums are formed of the ROUNDED r and y; a second-order term, parts in 10^4 of the bound)."""
import functools
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                                  # unit roundoff of fp32
SLOPE = np.float64(np.float32(0.01))            # LeakyReLU's slope as the kernels and the oracle hold it


def _f64(x):
    return np.asarray(x, np.float64)


def _cdiv(a, b):
    return (a + b - 1) // b


# ---- error bounds -----------------------------------------------------------------------------------------------------
# u = 2^-24.  A sum of n products formed in fp32, in any order, with or without fused multiply-adds, differs from the exact
# sum by at most gamma_n * sum |term_i| with gamma_n = n u / (1 - n u); (n + 2) u covers that for every n of these tests
# (n < 10^4) and leaves room for one rounding of an input factor (cw = deg * 0.01f).  A value that goes through one more
# fp32 operation gets one more u of its own magnitude.
def sum_bound(n, mag):
    """n: number of terms (scalar or array), mag: sum of the terms' magnitudes"""
    return (np.asarray(n, np.float64) + 2.0) * U * mag


def err_over_bound(got, ref, bound):
    """max over the elements of |got - ref| / bound; an element whose bound is 0 has to be exact"""
    got, ref, bound = _f64(got), _f64(ref), _f64(bound)
    if got.size == 0:
        return 0.0
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(d == 0, 0.0, d / bound)     # d > 0 over a bound of 0: inf
    return float(np.nan_to_num(q, nan=np.inf).max())


# ---- the graph side -----------------------------------------------------------------------------------------------------
def edge_owner(ptr):
    """the row / column every entry of a CSR / CSC pointer array belongs to"""
    ptr = np.asarray(ptr, np.int64)
    return np.repeat(np.arange(ptr.size - 1), np.diff(ptr))


def in_degrees(g):
    return np.diff(np.asarray(g["colPtr"], np.int64))


def expand_rows(colptr, row):
    """the per-edge tensor of a per-destination value"""
    return np.asarray(row).reshape(-1)[edge_owner(colptr)]


def rows_of_edges(colptr, x, fill=0.0):
    """the per-destination value of a per-edge tensor that is constant over every destination's edges (asserted, bit for
    bit); `fill` where a vertex has no in-edge"""
    ptr = np.asarray(colptr, np.int64)
    x = np.ascontiguousarray(x).reshape(-1)
    row = first_edge(ptr, x, fill)
    bits = (lambda v: v.view(np.uint32)) if x.dtype == np.float32 else (lambda v: v)
    assert np.array_equal(bits(x), bits(np.ascontiguousarray(expand_rows(ptr, row)))), "a per-edge tensor varies within a destination"
    return row


def first_edge(ptr, x, fill):
    """per destination, the value at its first in-edge (`fill` where it has none)"""
    ptr, x = np.asarray(ptr, np.int64), np.asarray(x).reshape(-1)
    out = np.full(ptr.size - 1, fill, x.dtype)
    has = ptr[1:] > ptr[:-1]
    out[has] = x[ptr[:-1][has]]
    return out


# ---- the stages ---------------------------------------------------------------------------------------------------------
def edge_forward(colptr, z, a):
    """edgNNForwardGAT: az[e] = z[dst(e), :] . a (an accumulator that starts at +0, as the oracle's does) and
    A[e] = az > 0 ? az : 0.01 az.  Returns dict(az, A, b_az, b_A), one entry per edge."""
    z, a = _f64(z), _f64(a).reshape(-1)
    F = z.shape[1]
    terms = z[edge_owner(colptr)] * a                       # E x F
    az = 0.0 + terms.sum(axis=1)
    b_az = sum_bound(F, np.abs(terms).sum(axis=1))
    pos = az > 0
    A = np.where(pos, az, SLOPE * az)
    b_A = np.where(pos, b_az, SLOPE * b_az + U * np.abs(A))  # the second operation: 0.01 * s
    return dict(az=az, A=A, b_az=b_az, b_A=b_A)


def edge_backward(colptr, grad, az, z, a):
    """edgNNBackwardGAT with the E x F dAct and the F x F z^T z built:
        dLRelu[e] = az[e] > 0 ? 1 : 0.01 ; dAct[e, :] = grad[dst(e), :] * dLRelu[e] ; dA[e] = dAct[e, :] . a
        r = sum_e dAct[e, :] (from 0) ; da = (z^T z) r
    Returns dict(dl, dA, b_dA, r, b_r, cw, da, b_da): dl, dA per edge; cw[v] = sum of dLRelu over v's in-edges (what the
    kernel keeps as deg * s_v); the bounds of r and da are those of r = grad^T cw, y = z r, da = z^T y, each composed from
    the one before with absolute values throughout."""
    grad, az, z, a = _f64(grad), _f64(az).reshape(-1), _f64(z), _f64(a).reshape(-1)
    N, F = z.shape
    own = edge_owner(colptr)
    dl = np.where(az > 0, 1.0, SLOPE)
    dAct = grad[own] * dl[:, None]                           # E x F
    t = dAct * a
    dA = 0.0 + t.sum(axis=1)
    b_dA = sum_bound(F + (dl != 1.0), np.abs(t).sum(axis=1))  # grad * 0.01f is rounded before it is multiplied
    r = 0.0 + dAct.sum(axis=0)
    npos = np.bincount(own, weights=(az > 0).astype(np.float64), minlength=N)
    cw = npos + (np.bincount(own, minlength=N) - npos) * SLOPE
    zz = z.T @ z                                             # F x F
    da = zz @ r
    az_, aw = np.abs(z), np.abs(grad).T @ np.abs(cw)
    b_r = sum_bound(N, aw)
    y = z @ r
    b_y = sum_bound(F, az_ @ (np.abs(r) + b_r)) + az_ @ b_r
    b_da = sum_bound(N, az_.T @ (np.abs(y) + b_y)) + az_.T @ b_y
    return dict(dl=dl, dA=dA, b_dA=b_dA, r=r, b_r=b_r, cw=cw, da=da, b_da=b_da)


def _gather_sum(N, own, w, rows):
    """S[v] = sum over the entries e of v of w[e] * rows[e], and the same sum of magnitudes"""
    T = rows * w[:, None] if w is not None else rows
    S, M = np.zeros((N, rows.shape[1])), np.zeros((N, rows.shape[1]))
    if T.shape[0]:
        np.add.at(S, own, T)
        np.add.at(M, own, np.abs(T))
    return S, M


def _stack(local, ghost, use_ghosts=True):
    """local rows, then ghost rows (as zeros with use_ghosts = False: the sensitivity premise's "ghost rows omitted")"""
    local = _f64(local)
    if ghost is None or not np.size(ghost):
        return local
    gh = _f64(ghost)
    return np.vstack([local, gh if use_ghosts else np.zeros_like(gh)])


def neighbour_sum(g, z, fgz, use_ghosts=True):
    """S[v] = sum over v's in-edges of z_src (ghost sources included): tensor "nsum".  Returns (S, bound)."""
    N = g["localVtxCnt"]
    S, M = _gather_sum(N, edge_owner(g["colPtr"]), None, _stack(z, fgz, use_ghosts)[np.asarray(g["rowIdx"], np.int64)])
    return S, sum_bound(in_degrees(g)[:, None], M)


def aggregate_fwd(g, A, z, fgz, use_ghosts=True, drop=None):
    """aggregateGAT forward: ah[v] = z[v] + sum over in-edges of A[e] z_src(e).  `drop`: a boolean mask of in-edges left
    out (the sensitivity premise).  The bound: deg + 1 terms, then the row scaling and the addition of the forms that make
    ah = z + arow * S of the unweighted sum S -- one u of the scaled sum and one of ah."""
    N = g["localVtxCnt"]
    A = _f64(A).reshape(-1)
    if drop is not None:
        A = np.where(drop, 0.0, A)
    z = _f64(z)
    S, M = _gather_sum(N, edge_owner(g["colPtr"]), A, _stack(z, fgz, use_ghosts)[np.asarray(g["rowIdx"], np.int64)])
    ah = z + S
    return ah, sum_bound(in_degrees(g)[:, None] + 1, np.abs(z) + M) + U * np.abs(S) + U * np.abs(ah)


def aggregate_bwd(g, grad, bgd, dA, z, fgz, use_ghosts=True, drop=None):
    """aggregateGAT backward, the fresh two-term sum: aTg[v] = sum over out-edges of csrVal[e] grad_dst(e) + sum over
    in-edges of dA[e] z_src(e).  The bound follows the cancellation between the two terms: it is made of the magnitudes
    summed, plus one u of the second term (its row scaling) and one of aTg (the addition of the two)."""
    N = g["localVtxCnt"]
    dA = _f64(dA).reshape(-1)
    if drop is not None:
        dA = np.where(drop, 0.0, dA)
    S1, M1 = _gather_sum(N, edge_owner(g["rowPtr"]), _f64(g["csrVal"]), _stack(grad, bgd, use_ghosts)[np.asarray(g["colIdx"], np.int64)])
    S2, M2 = _gather_sum(N, edge_owner(g["colPtr"]), dA, _stack(z, fgz, use_ghosts)[np.asarray(g["rowIdx"], np.int64)])
    n = (in_degrees(g) + np.diff(np.asarray(g["rowPtr"], np.int64)))[:, None]
    aTg = S1 + S2
    return aTg, sum_bound(n, M1 + M2) + U * np.abs(S2) + U * np.abs(aTg)


# ---- launch_colsum_w's plan (csrc/elementwise.hip) -------------------------------------------------------------------------
# test_gat_stage_reference.py reads these constants out of elementwise.hip: a retuned plan fails there and points here.
COLSUM_MAX_BLOCKS = 512        # first-stage workgroups at the most
COLSUM_MIN_ROWS = 64           # ... of at least this many rows each
COLSUM_THREADS = 256           # threads of a first-stage workgroup: float4 columns x row groups
FINAL_COLS, FINAL_GROUPS = 32, 8   # second stage: 32 columns x 8 groups of partials per workgroup
LANES = 64                     # the wave-per-row kernels' lane loops (j += 64) and edge loops (e += 64)
ROWS_PER_WORKGROUP = 4         # ... and their four rows per 256-thread workgroup
SCRATCH_PARTIAL_ROWS = 1024    # dory_apply_edge sizes the partial buffer for this many blocks: the cap by bytes never binds


def colsum_plan(N, F):
    """what launch_colsum_w and its two kernels do with an N x F tensor"""
    nb = COLSUM_MAX_BLOCKS
    while nb > 1 and nb > N // COLSUM_MIN_ROWS:
        nb >>= 1
    rpb = max(_cdiv(N, nb), 1)
    nb = max(_cdiv(N, rpb), 1)
    F4 = _cdiv(F, 4)
    CW = min(F4, COLSUM_THREADS)
    RG = COLSUM_THREADS // CW
    return dict(nb=nb, rows_per_block=rpb, last_block_rows=N - (nb - 1) * rpb, F4=F4, CW=CW, RG=RG, idle=COLSUM_THREADS - CW * RG,
                passes=_cdiv(F4, CW), tail_live=F % 4 != 0, final_trips=_cdiv(nb, FINAL_GROUPS), final_blocks=_cdiv(F, FINAL_COLS))


# ---- the cases ------------------------------------------------------------------------------------------------------------
NS = [1, 2, 3, 5, 63, 64, 65, 300, 1100]
FS = [2, 6, 41, 63, 64, 65, 128, 602, 1028]
PINNED_DEGREES = [0, 1, 63, 64, 65]
HUB = 230
# (N, F) of the edge stage: every N at a narrow and at an odd width, every F at one workgroup of rows and at several, and the
# 16-block plan (ragged last block, two trips of the second stage) at the widths its sensitivity premise holds for.  A width of
# 1 is a case of its own (WIDTH_ONE): such tensors keep ld = 1.
EDGE_CASES = sorted(set([(n, 6) for n in NS] + [(n, 41) for n in NS] + [(65, f) for f in FS] + [(300, f) for f in FS] + [(1100, 65)]))
WIDTH_ONE = (65, 1)
# (N, F) of the aggregations (graphs of make_graph) and (golden, F) with ghost rows
AGG_CASES = [(65, 6), (65, 41), (300, 41), (300, 128), (1100, 65)]
AGG_GOLDENS = [("parts_toy60_p2", 41), ("parts_toy60_p4_hash", 16)]
FAMILIES = ["dyadic", "random"]
SIGN_ROLES = ["zero", "negzero", "pos", "neg"]


def case_degrees(N):
    """in-degrees of make_graph(N): the pinned classes and a hub where the graph is large enough, small ones elsewhere; the
    LAST vertex carries the hub, so that the last row of a ragged colsum block weighs in r"""
    rng = np.random.default_rng([7, N])
    deg = rng.integers(0, 6, N)
    if N >= 63:
        deg[:5] = PINNED_DEGREES
        deg[5] = 0                      # a second vertex nobody points to, away from the first workgroup's first wave
    else:
        deg[0] = 0
        if N > 1:
            deg[1:] = np.maximum(deg[1:], 1)
    if N >= 300:
        deg[N - 1] = HUB
    elif N > 1:
        deg[N - 1] = max(deg[N - 1], 2)
    if N == 1:
        deg[:] = 0                      # the loader drops self loops: a lone vertex has no edge
    return deg


def make_graph(N, undirected=False):
    """(src, dst, parts) of one partition with case_degrees(N): sources drawn among the other vertices (an edge may repeat:
    the loader keeps every record), records shuffled"""
    deg = case_degrees(N)
    rng = np.random.default_rng([8, N])
    dst = np.repeat(np.arange(N), deg)
    src = (dst + 1 + rng.integers(0, max(N - 1, 1), dst.size)) % max(N, 1)
    p = rng.permutation(dst.size)
    return src[p].astype(np.uint32), dst[p].astype(np.uint32), np.zeros(N, np.int64)


def shape_classes(N, F, deg):
    """the classes of the issue's list an (N, F) case with in-degrees `deg` reaches"""
    p, c = colsum_plan(N, F), set()
    c.add(f"N={N}")
    c.add(f"F={F}")
    if N % ROWS_PER_WORKGROUP:
        c.add("row_guard_live")                  # v >= N in the last workgroup of the wave-per-row kernels
    if F > LANES:
        c.add("lane_loop_second_trip")
    if p["idle"]:
        c.add("colsum_idle_threads")
    if p["tail_live"]:
        c.add("colsum_tail_live")
    if F % 4 == 1:
        c.add("F%4==1")
    if p["passes"] > 1:
        c.add("colsum_second_pass")
    if p["nb"] > 4:
        c.add("colsum_more_than_4_blocks")
    if p["final_trips"] > 1:
        c.add("final_second_trip")
    if p["nb"] > 1 and p["last_block_rows"] != p["rows_per_block"]:
        c.add("ragged_last_block")
    for d in PINNED_DEGREES:
        if (deg == d).any():
            c.add(f"deg={d}")
    if (deg >= 200).any():
        c.add("hub")
    return c


REQUIRED_SHAPE_CLASSES = ([f"N={n}" for n in NS] + [f"F={f}" for f in FS] + [f"deg={d}" for d in PINNED_DEGREES] +
                          ["hub", "row_guard_live", "lane_loop_second_trip", "colsum_idle_threads", "colsum_tail_live", "F%4==1",
                           "colsum_second_pass", "colsum_more_than_4_blocks", "final_second_trip", "ragged_last_block"])
REQUIRED_SIGN_CLASSES = ["az>0", "az<0", "az=+0 of a zero row", "az=+0 of a -0.0 row", "uploaded az: +", "uploaded az: -",
                         "uploaded az: +0", "uploaded az: -0.0"]


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def _draw(rng, family, shape):
    if family == "dyadic":     # multiples of 1/64 in [-1, 1]: every dot product of up to 4096 of them is exact in fp32, in any order
        return (rng.integers(-64, 65, shape) / 64.0).astype(np.float32)
    return rng.uniform(-1, 1, shape).astype(np.float32)


def sign_roles(deg):
    """which vertex plays which sign role: the first four vertices with in-edges, in SIGN_ROLES' order (with the pinned
    degrees: 1, 63, 64 and 65 in-edges)"""
    has = np.nonzero(np.asarray(deg) > 0)[0]
    return {role: int(v) for role, v in zip(SIGN_ROLES, has)}


MARGIN = 16.0


def margin_ok(z, a):
    """the sign margin per ROW of z: |az| > 16 bound(az), or az == 0 exactly (float64)"""
    z, a = _f64(z), _f64(a).reshape(-1)
    t = z * a
    az = t.sum(axis=1)
    return (az == 0) | (np.abs(az) > MARGIN * sum_bound(z.shape[1], np.abs(t).sum(axis=1)))


def stage_inputs(g, F, family, seed=0):
    """z, fg_z, grad, bg_d, a and a caller's az (per edge, constant per destination, signs unrelated to the computed ones, with
    +0 and -0.0 among them) for one partition.  The sign roles: a z row of +0 and one of -0.0 (az = +0 both: the sum starts at
    +0), a row with the signs of a (az > 0 whatever the rounding) and one against them; the grad rows of the first two follow
    the signs of a, so that the branch az = 0 takes is visible in dA.  Random family: a row whose az is closer to 0 than the
    margin is drawn again -- a property of the inputs, asserted by test_gat_stage_reference.py for every case."""
    N, deg = g["localVtxCnt"], in_degrees(g)
    rng = np.random.default_rng([seed, N, F, FAMILIES.index(family), g["srcGhostCnt"], int(np.asarray(g["colPtr"])[-1])])
    z, grad = _draw(rng, family, (N, F)), _draw(rng, family, (N, F))
    fgz, bgd = _draw(rng, family, (g["srcGhostCnt"], F)), _draw(rng, family, (g["dstGhostCnt"], F))
    a = _draw(rng, family, (F, 1))
    a[a == 0] = np.float32(1 / 64)
    sa = np.sign(a.reshape(-1)).astype(np.float32)
    nz = lambda x: np.where(x == 0, np.float32(1 / 64), np.abs(x)).astype(np.float32)
    roles = sign_roles(deg)
    for role, v in roles.items():
        if role == "zero":
            z[v] = 0.0
        elif role == "negzero":
            z[v] = -0.0
        elif role == "pos":
            z[v] = sa * nz(z[v])
        else:
            z[v] = -sa * nz(z[v])
        if role in ("zero", "negzero"):
            grad[v] = sa * np.maximum(nz(grad[v]), np.float32(0.25))
    if N and deg[N - 1] >= 200:
        # the hub is the last vertex: its rows of z and grad are the signs of a at full size, so that az > 0, r is close to
        # HUB * sign(a) and y = z r is largest at the last row -- the row a ragged last colsum block would lose weighs in both sums
        z[N - 1] = sa
        grad[N - 1] = sa
    if family == "random":
        for _ in range(200):
            bad = np.nonzero(~margin_ok(z, a))[0]
            if not bad.size:
                break
            z[bad] = _draw(rng, family, (bad.size, F))
    az_row = _draw(rng, family, N)
    az_row[az_row == 0] = np.float32(0.5)
    if N > 0:
        az_row[rng.permutation(N)[:max(N // 8, 1)]] = np.float32(0.0)
        if N > 1:
            az_row[rng.permutation(N)[:max(N // 8, 1)]] = np.float32(-0.0)
    return dict(z=z, fg_z=fgz, grad=grad, bg_d=bgd, a=a, az_up=expand_rows(g["colPtr"], az_row).astype(np.float32), roles=roles)


def sign_classes(g, inp):
    """the sign classes a case's inputs reach (float64 reference)"""
    fw = edge_forward(g["colPtr"], inp["z"], inp["a"])
    own, c = edge_owner(g["colPtr"]), set()
    if (fw["az"] > 0).any():
        c.add("az>0")
    if (fw["az"] < 0).any():
        c.add("az<0")
    for role, name in (("zero", "az=+0 of a zero row"), ("negzero", "az=+0 of a -0.0 row")):
        v = inp["roles"].get(role)
        if v is not None and (own == v).any() and (fw["az"][own == v] == 0).all() and not np.signbit(fw["az"][own == v]).any():
            c.add(name)
    up = inp["az_up"]
    for name, m in (("+", up > 0), ("-", up < 0), ("+0", (up == 0) & ~np.signbit(up)), ("-0.0", (up == 0) & np.signbit(up))):
        if m.any():
            c.add("uploaded az: " + name)
    return c


# ---- the prototype's epoch over partitions, float64 -------------------------------------------------------------------------
def softmax64(x):
    """orc_softmax: max-subtracted, the denominator seeded with 1e-20f"""
    x = _f64(x)
    if x.shape[0] == 0:
        return x.copy()
    e = np.exp(x - x.max(axis=1, keepdims=True))
    return e / (e.sum(axis=1, keepdims=True) + np.float64(np.float32(1e-20)))


def gat_epoch_parts(gs, H0, labels, Ws, As):
    """helpers.oracle_gat_epoch_parts in float64: same stage order, same ghost exchange, every stage one of the references
    above.  Returns the per-partition tensor dicts."""
    P, L = len(gs), len(Ws)
    g2l = {}
    for r, g in enumerate(gs):
        for l, gv in enumerate(g["localToGlobal"]):
            g2l[int(gv)] = (r, l)

    def ghosts(key, tensors):
        F = tensors[0].shape[1]
        return [np.asarray([tensors[g2l[int(gv)][0]][g2l[int(gv)][1]] for gv in g[key]], np.float64).reshape(len(g[key]), F) for g in gs]

    T = [dict() for _ in range(P)]
    feats = [_f64(H0)[np.asarray(g["localToGlobal"], np.int64)] for g in gs]
    for l in range(L):
        zs = [feats[r] @ _f64(Ws[l]) for r in range(P)]
        fgz = ghosts("srcGhost", zs)
        nf = []
        for r, g in enumerate(gs):
            fw = edge_forward(g["colPtr"], zs[r], As[l])
            ah, _ = aggregate_fwd(g, fw["A"], zs[r], fgz[r])
            T[r].update({f"in{l}": feats[r], f"z{l}": zs[r], f"fg_z{l}": fgz[r], f"az{l}": fw["az"], f"A{l}": fw["A"], f"ah{l}": ah})
            nf.append(ah)
        feats = nf
    C = np.asarray(Ws[-1]).shape[1]
    grads = [softmax64(feats[r]) - np.eye(C)[np.asarray(labels)[np.asarray(g["localToGlobal"], np.int64)]] for r, g in enumerate(gs)]
    for l in range(L - 1, -1, -1):
        bgd = ghosts("dstGhost", grads)
        ngr = []
        for r, g in enumerate(gs):
            bw = edge_backward(g["colPtr"], grads[r], T[r][f"az{l}"], T[r][f"z{l}"], As[l])
            aTg, _ = aggregate_bwd(g, grads[r], bgd[r], bw["dA"], T[r][f"z{l}"], T[r][f"fg_z{l}"])
            T[r].update({f"grad{l}": grads[r], f"bg_d{l}": bgd[r], f"dA{l}": bw["dA"], f"aTg{l}": aTg, f"da{l}": bw["da"]})
            ngr.append(aTg @ _f64(Ws[l]).T if l > 0 else None)
        grads = ngr
    return T


# ---- the graphs of the cases (shared by the two test files) -------------------------------------------------------------------
EDGE_IDS = [f"N{n}-F{f}" for n, f in EDGE_CASES]


@functools.lru_cache(maxsize=None)
def graph(N):
    """the single partition of make_graph(N), built by the partition oracle"""
    import partition_oracle as po
    s, d, parts = make_graph(N)
    return po.preprocess(s, d, parts, 0, 1)


@functools.lru_cache(maxsize=None)
def golden(name):
    """every rank of a committed golden partition set"""
    import partition_oracle as po
    bins = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", name, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    return [po.parse_graph_bin(open(b, "rb").read()) for b in bins]


def golden_parts(name):
    return np.loadtxt(os.path.join(ROOT, "tests", "golden", name, "graph.bsnap.parts"), dtype=np.int64, ndmin=1)


OPEN_CASE, OPEN_DIMS, OPEN_SEED = "parts_toy60_p4_hash", [20, 16, 6], 11


def open_case_inputs(case=OPEN_CASE):
    """the setup of test_gat_epoch_partitions_vs_oracle (dims [20, 16, 6], seed 11) on a golden: partitions, parts, H0, labels,
    Ws, As"""
    gs, dims = golden(case), OPEN_DIMS
    V = int(gs[0]["globalVtxCnt"])
    rng = np.random.default_rng(OPEN_SEED)
    H0 = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(2)]
    As = [(rng.standard_normal((dims[i + 1], 1)) / 2).astype(np.float32) for i in range(2)]
    return gs, golden_parts(case), H0, labels, Ws, As
