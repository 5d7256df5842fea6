"""The aggregation stage in plain float64 -- out[v] = self * xl[v] + sum_e val[e] * row(idx[e]) -- with inputs that make every
fp32 partial sum exact, graph builders that take arbitrary edge values, a Python mirror of the dispatch in csrc/abi_stages.hip
(which kernel family runs, in which form) and the case list the aggregation tests share.

tests/test_gpu_aggregate_stage.py compares K1 / K1b / K1s with these references bit for bit; tests/test_aggregate_stage_reference.py
compares the reference with the committed C oracle and the mirror's constants with the sources, and proves that the case list
reaches every form -- where there is no GPU."""
import functools

import numpy as np
import scipy.sparse as sp

# ---- constants of the kernels (test_aggregate_stage_reference.py reads them out of the sources) ---------------------------------
LONG_ROW_CLAMP, LONG_ROW_CHUNK = 8192, 4096      # ctx.hpp: K1's long rows
BLK_SEG_CLAMP, BLK_SEG_CHUNK = 2048, 4096        # ctx.hpp: K1b's long (block, row) segments
BLK_ROWS = 32                                    # spmm_blocked.hip: destination rows per K1b workgroup
SWEEP_SPLIT = 2                                  # spmm.hip: rows beyond SWEEP_SPLIT x the mean degree are cut into pieces
SWEEP_SPLIT_MIN = 64
SWEEP_C = 128                                    # sweep_core.hpp: staged entries per lane group and pass (a pass holds SWEEP_C - 1)
SWEEP_NT = 1024                                  # threads of a K1s workgroup
TINY_BYTES = 4 << 20                             # the whole source slab in one L2: K1
SWEEP_MAX_NB, BLOCKED_MAX_NB = 512, 256
OFFSET_TABLE_BYTES = 8 << 30
SWEEP_WINDOW_KB_FEW_ROWS, SWEEP_WINDOW_KB = 3584, 2432   # ensure_sweep: R <= 4 / otherwise
BLOCKED_WINDOW_WIDE, BLOCKED_WINDOW_NARROW = 5242880, 3932160   # plan_blocks: rows of >= 512 bytes / narrower
K1_TABLE = [(8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (96, 32, 3), (128, 64, 2), (192, 64, 3), (None, 64, 4)]   # launch_spmm: chunks <=, GROUP, CHUNKS
K1_FORMS = [(g, c) for _, g, c in K1_TABLE]
PICK_R = [10, 8, 6, 4, 2]                        # sweep_pick_r's candidates, in its order
K1S_FORMS = [(32, r) for r in (2, 4, 6, 8, 10)] + [(16, r) for r in (2, 3, 4, 5, 6, 8)]   # the instantiated (GROUP, R)
CUS_PER_XCD = 32                                 # what the mirror assumes of the device (256 CUs in 8 XCDs)
LOADER_RELIEF = 3                                # option spmm_sweep_loader_relief's default

DEFAULTS = dict(spmm_variant=2, spmm_blk_nb=0, spmm_blk_group=32, spmm_blk_force_split=0, spmm_order=1, spmm_slab=0,
                spmm_edge_split=1, spmm_sweep_rows=0, spmm_sweep_pair=-1, spmm_sweep_loader=1, spmm_sweep_layout=3,
                spmm_sweep_window_kb=0, gcn_bf16_gather=0)


def _cdiv(a, b):
    return (a + b - 1) // b


def pad_ld(cols):
    return cols if cols <= 1 else (cols + 31) // 32 * 32


# ---- the float64 reference ----------------------------------------------------------------------------------------------------------
def _rows64(xl, xg):
    xl = np.asarray(xl, np.float64)
    if xg is None or len(xg) == 0:
        return xl
    return np.vstack([xl, np.asarray(xg, np.float64)])


def _matrix(ptr, idx, val, ncols):
    ptr = np.asarray(ptr, np.int64)
    return sp.csr_matrix((np.asarray(val, np.float64), np.asarray(idx, np.int64), ptr), shape=(ptr.size - 1, ncols))


def _self_term(self_scale, xl, self_mode, N):
    x = np.asarray(xl, np.float64)[:N]
    if self_mode == 0:
        return np.zeros_like(x)
    return x * np.asarray(self_scale, np.float64)[:, None] if self_mode == 1 else x.copy()


def aggregate(ptr, idx, val, self_scale, xl, xg, self_mode):
    """out[v] = self * xl[v] + sum over e in [ptr[v], ptr[v+1]) of val[e] * row(idx[e]); row(i) = xl[i] if i < N else xg[i - N];
    self = 0 / self_scale[v] / 1 for self_mode 0 / 1 / 2 (csrc/spmm.hip's header).  float64; duplicate entries are summed"""
    X = _rows64(xl, xg)
    N = len(ptr) - 1
    return _self_term(self_scale, xl, self_mode, N) + _matrix(ptr, idx, val, X.shape[0]) @ X


def magnitude(ptr, idx, val, self_scale, xl, xg, self_mode):
    """|self * x[v]| + sum |val[e]| * |row(idx[e])|, per element: what a rounding error of the sum is relative to"""
    X = np.abs(_rows64(xl, xg))
    N = len(ptr) - 1
    return np.abs(_self_term(self_scale, xl, self_mode, N)) + _matrix(ptr, idx, np.abs(np.asarray(val, np.float64)), X.shape[0]) @ X


def fp32_sum_bound(ptr, idx, val, self_scale, xl, xg, self_mode):
    """the bound on |fp32 result - exact| of a sum of n + 1 fused terms taken in ANY order (Higham, Accuracy and Stability of
    Numerical Algorithms, 3.1 / 4.2: every term passes through at most n + 1 roundings, one more for a final scaling or
    accumulation): gamma * magnitude with gamma = (n + 2) u / (1 - (n + 2) u), u = 2^-24, n = the row's degree"""
    n = np.diff(np.asarray(ptr, np.int64)).astype(np.float64)
    u = 2.0 ** -24
    gamma = (n + 2) * u / (1 - (n + 2) * u)
    return gamma[:, None] * magnitude(ptr, idx, val, self_scale, xl, xg, self_mode)


def bf16_round(x):
    """fp32 -> bf16 -> fp32, round to nearest even (the conversion of launch_bf16_rows), finite values"""
    b = np.ascontiguousarray(x, np.float32).view(np.uint32).astype(np.uint64)
    b = (b + 0x7FFF + ((b >> 16) & 1)) & 0xFFFF0000
    return b.astype(np.uint32).view(np.float32).reshape(np.shape(x))


# ---- exact inputs -------------------------------------------------------------------------------------------------------------------------
INT_MAX = 8                                       # features: integers in -8..8 (exact in bf16 too)
WEIGHTS = np.array([s * m for s in (1.0, -1.0) for m in (0.25, 0.5, 1.0, 2.0)], np.float32)   # signed powers of two


def exact_features(rng, rows, F):
    return rng.integers(-INT_MAX, INT_MAX + 1, (rows, F)).astype(np.float32)


def exact_weights(rng, n):
    """one draw per edge: equal weights would hide a swapped (idx, val) pair"""
    return WEIGHTS[rng.integers(0, WEIGHTS.size, n)]


def exact_ok(ptr, idx, val, self_scale, xl, xg, self_mode):
    """asserts what makes the order of the additions irrelevant: the weights are signed powers of two down to 1/4 and the
    features integers, so every partial sum of every subset of a row's terms is a multiple of 1/4; it is exact in fp32 (24
    bits) if it stays below 2^22, i.e. if 4 * (|self * x| + sum |val| |x|) < 2^24 per element"""
    assert np.isin(np.abs(np.asarray(val, np.float32)), [0.25, 0.5, 1.0, 2.0]).all()
    if self_mode == 1:
        assert np.isin(np.abs(np.asarray(self_scale, np.float32)), [0.25, 0.5, 1.0, 2.0]).all()
    for x in (xl, xg):
        if x is not None and len(x):
            assert (np.asarray(x) == np.rint(x)).all() and np.abs(x).max() <= INT_MAX
    m = magnitude(ptr, idx, val, self_scale, xl, xg, self_mode)
    worst = float(m.max()) if m.size else 0.0
    assert 4 * worst < 2 ** 24, worst
    return worst


# ---- graphs -------------------------------------------------------------------------------------------------------------------------------
def _csr_of(rows, cols, w, N):
    o = np.argsort(rows, kind="stable")           # the edge list's order inside every row
    ptr = np.zeros(N + 1, np.uint64)
    ptr[1:] = np.cumsum(np.bincount(rows, minlength=N))
    return ptr, cols[o].astype(np.uint32), w[o].astype(np.float32)


def graph_from_edges(N, Gs, Gd, s, d, w, norm):
    """the dict Context.graph_upload takes, from an edge list with arbitrary values.  s in [0, N + Gs): local sources and ghost
    sources N + k; d in [0, N + Gd) likewise; no edge joins two ghosts.  The CSC holds the edges with a local destination (by
    destination, edge-list order inside), the CSR those with a local source: a local-local edge carries the same value in
    both.  Nothing is merged or dropped: multi-edges and self loops stay"""
    s, d, w = np.asarray(s, np.int64), np.asarray(d, np.int64), np.asarray(w, np.float32)
    assert s.size == d.size == w.size and not ((s >= N) & (d >= N)).any()
    assert (s >= 0).all() and (s < N + Gs).all() and (d >= 0).all() and (d < N + Gd).all()
    i, o = d < N, s < N
    colPtr, rowIdx, cscVal = _csr_of(d[i], s[i], w[i], N)
    rowPtr, colIdx, csrVal = _csr_of(s[o], d[o], w[o], N)
    return dict(localVtxCnt=N, globalVtxCnt=N + max(Gs, Gd), srcGhostCnt=Gs, dstGhostCnt=Gd, colPtr=colPtr, rowIdx=rowIdx,
                cscVal=cscVal, rowPtr=rowPtr, colIdx=colIdx, csrVal=csrVal, norm=np.asarray(norm, np.float32))


def split_deg(nnz, N):
    """build_blocked_sweep: rows of more edges are cut into pieces"""
    return max(SWEEP_SPLIT_MIN, SWEEP_SPLIT * (nnz // N + 1))


# degrees planted on both sides, each row's degree exactly this (tests/test_aggregate_stage_reference.py asserts the list
# against the kernels' boundaries)
PLANTED_SHORT = ([0, 1, 3, 4, 5] + [g + k for g in (8, 16, 32, 64) for k in (-1, 0, 1)] +
                 [SWEEP_C - 2, SWEEP_C - 1, SWEEP_C, SWEEP_C + 1])
PLANTED_SEGMENTS = [BLK_SEG_CLAMP, BLK_SEG_CLAMP + 1, BLK_SEG_CLAMP + BLK_SEG_CHUNK, BLK_SEG_CLAMP + BLK_SEG_CHUNK + 1]
PLANTED_LONG = ([LONG_ROW_CLAMP, LONG_ROW_CLAMP + 1, LONG_ROW_CLAMP + 2, LONG_ROW_CLAMP + 3,            # a chunk of 1, 2, 3 edges
                 LONG_ROW_CLAMP + LONG_ROW_CHUNK, LONG_ROW_CLAMP + LONG_ROW_CHUNK + 1,
                 LONG_ROW_CLAMP + LONG_ROW_CHUNK + 2, LONG_ROW_CLAMP + LONG_ROW_CHUNK + 3,
                 LONG_ROW_CLAMP + 2 * LONG_ROW_CHUNK + 1001,                                           # remainder not a multiple of 4
                 LONG_ROW_CLAMP + 6 * LONG_ROW_CHUNK + 77])
# lane groups of four consecutive rows whose entries of one step sum to SWEEP_C - 2 .. SWEEP_C + 1 (and to half of that: a 16-lane
# launch with the loader wave stages SWEEP_C / 2 per pass): graph "staging", swept in row order over ONE source block
# (spmm_sweep_layout = 0, spmm_blk_nb = 1, spmm_sweep_rows = 4), so that a group's step holds exactly its rows' edges
PLANTED_STAGING = [32, 32, 31, 31, 32, 32, 32, 31, 32, 32, 32, 32, 33, 32, 32, 32, 64, 63, 0, 0, 64, 64, 0, 0, 1, 0, 64, 64,
                   16, 16, 15, 15, 16, 16, 16, 15, 16, 16, 16, 16, 17, 16, 16, 16, 0, 0, 0, 0]
HUNDREDS_OF_PIECES = 300                          # a row of this many pieces of split_deg edges


def _plant(rng, N, free_lo, degrees, narrow):
    """`degrees[i]` edges into planted vertex i from sources in the unplanted range [free_lo, N) (narrow: from its first 64
    vertices, so that the row's edges fall into one source block of K1b's layout)"""
    rows = np.repeat(np.arange(len(degrees), dtype=np.int64), degrees)
    hi = free_lo + 64 if narrow else N
    return rows, rng.integers(free_lo, hi, rows.size)


def _structure(name):
    """(N, Gs, Gd, s, d, planted) of a named graph; planted = {side: {vertex: degree}} for the rows whose degree is exact"""
    rng = np.random.default_rng([17, sum(name.encode())])
    kind, _, arg = name.partition(":")
    if kind == "uniform":                         # "uniform:N:E"
        N, E = (int(x) for x in arg.split(":"))
        return N, 0, 0, rng.integers(0, N, E), rng.integers(0, N, E), {}
    if kind == "powerlaw":                        # both sides skewed, hubs at scattered ids
        N, E = (int(x) for x in arg.split(":"))
        ps, pd = rng.permutation(N), rng.permutation(N)
        return N, 0, 0, ps[(N * rng.random(E) ** 3).astype(np.int64)], pd[(N * rng.random(E) ** 3).astype(np.int64)], {}
    if kind == "multi":                           # multi-edges (every edge one to four times, not adjacent) and self loops
        N, E = (int(x) for x in arg.split(":"))
        s, d = rng.integers(0, N, E), rng.integers(0, N, E)
        loops = rng.integers(0, N, N // 2)
        s, d = np.concatenate([s, loops, s[: E // 2], s[: E // 4], s[: E // 8]]), np.concatenate([d, loops, d[: E // 2], d[: E // 4], d[: E // 8]])
        o = rng.permutation(s.size)
        return N, 0, 0, s[o], d[o], {}
    if kind == "planted":                         # exact degrees on both sides, below the long-row clamp
        N, mean = 24000, 36
        n_in = len(PLANTED_SHORT) + len(PLANTED_SEGMENTS) + 2
        P = 2 * n_in                               # vertices [0, n_in): planted in-degree; [n_in, P): planted out-degree
        E0 = (N - P) * mean
        fixed = sum(PLANTED_SHORT) + sum(PLANTED_SEGMENTS)
        sd = SWEEP_SPLIT_MIN
        while split_deg(E0 + 2 * (fixed + 2 * sd + 1), N) != sd:
            sd += 1
        degs = PLANTED_SHORT + PLANTED_SEGMENTS + [sd, sd + 1]
        narrow = [False] * len(PLANTED_SHORT) + [True] * len(PLANTED_SEGMENTS) + [False, False]
        bs, bd = rng.integers(P, N, E0), rng.integers(P, N, E0)
        parts_s, parts_d = [bs], [bd]
        for side in (0, 1):
            for nar in (False, True):
                sel = [dg if nr == nar else 0 for dg, nr in zip(degs, narrow)]
                rows, other = _plant(rng, N, P, sel, nar)
                rows = rows + side * n_in
                parts_s.append(other if side == 0 else rows)
                parts_d.append(rows if side == 0 else other)
        s, d = np.concatenate(parts_s), np.concatenate(parts_d)
        o = rng.permutation(s.size)
        planted = {"in": {i: dg for i, dg in enumerate(degs)}, "out": {n_in + i: dg for i, dg in enumerate(degs)}}
        return N, 0, 0, s[o], d[o], planted
    if kind == "staging":
        N, degs = 4096, PLANTED_STAGING
        n_in = len(degs)
        P = 2 * n_in
        parts_s, parts_d = [rng.integers(P, N, 60000)], [rng.integers(P, N, 60000)]
        for side in (0, 1):
            rows, other = _plant(rng, N, P, degs, False)
            rows = rows + side * n_in
            parts_s.append(other if side == 0 else rows)
            parts_d.append(rows if side == 0 else other)
        s, d = np.concatenate(parts_s), np.concatenate(parts_d)
        o = rng.permutation(s.size)
        return N, 0, 0, s[o], d[o], {"in": dict(enumerate(degs)), "out": {n_in + i: dg for i, dg in enumerate(degs)}}
    if kind == "hubs":                            # a few hubs beyond every clamp, most rows empty
        N = 12000
        sd = SWEEP_SPLIT_MIN                       # (mean degree stays far below 32: checked by the CPU test)
        degs = PLANTED_LONG + [HUNDREDS_OF_PIECES * sd]
        n_in = len(degs)
        P = 2 * n_in
        parts_s, parts_d = [], []
        live = rng.permutation(np.arange(P, N))[: (N - P) * 3 // 10]       # seven of ten unplanted rows stay empty on both sides
        E0 = 20000
        parts_s.append(live[rng.integers(0, live.size, E0)])
        parts_d.append(live[rng.integers(0, live.size, E0)])
        for side in (0, 1):
            rows, other = _plant(rng, N, P, degs, False)
            rows, other = rows + side * n_in, live[other % live.size]     # (the hubs' neighbours are live rows too)
            parts_s.append(other if side == 0 else rows)
            parts_d.append(rows if side == 0 else other)
        s, d = np.concatenate(parts_s), np.concatenate(parts_d)
        o = rng.permutation(s.size)
        planted = {"in": {i: dg for i, dg in enumerate(degs)}, "out": {n_in + i: dg for i, dg in enumerate(degs)}}
        return N, 0, 0, s[o], d[o], planted
    if kind == "ghosts":                          # "ghosts:N:Gs:Gd:E_local:E_in:E_out": one partition with ghost rows on both sides
        N, Gs, Gd, El, Ei, Eo = (int(x) for x in arg.split(":"))
        q = N // 4
        # destinations [0, q) have ghost sources only, [q, 2q) local sources only, the rest both; the same for the sources'
        # out-edges (rows with no local neighbour, rows with no ghost neighbour)
        ls, ld = rng.integers(0, N, El), rng.integers(q, N, El)
        keep = ls >= q                             # (sources [0, q) reach ghosts only)
        ls, ld = ls[keep], ld[keep]
        gi_s, gi_d = N + rng.integers(0, max(Gs, 1), Ei), np.where(rng.random(Ei) < 0.3, rng.integers(0, q, Ei), rng.integers(2 * q, N, Ei))
        go_d, go_s = N + rng.integers(0, max(Gd, 1), Eo), np.where(rng.random(Eo) < 0.3, rng.integers(0, q, Eo), rng.integers(2 * q, N, Eo))
        s, d = np.concatenate([ls, gi_s, go_s]), np.concatenate([ld, gi_d, go_d])
        o = rng.permutation(s.size)
        return N, Gs, Gd, s[o], d[o], {}
    raise KeyError(name)


@functools.lru_cache(maxsize=8)
def graph(name, values="exact"):
    """the named graph as a graph_upload dict.  values = "exact": weights and norm drawn from WEIGHTS; "real": GCN's symmetric
    normalisation 1 / sqrt((deg_s + 1)(deg_d + 1)) from the graph's own degrees (ghosts: a drawn degree), norm = 1 / (deg + 1)"""
    N, Gs, Gd, s, d, planted = _structure(name)
    rng = np.random.default_rng([23, sum(name.encode()), len(values)])
    if values == "exact":
        w, norm = exact_weights(rng, s.size), exact_weights(rng, N)
    else:
        deg_d = np.concatenate([np.bincount(d[d < N], minlength=N), rng.integers(1, 60, Gd)]).astype(np.float64)
        deg_s = np.concatenate([deg_d[:N], rng.integers(1, 60, Gs)])
        w = (1.0 / np.sqrt((deg_s[s] + 1) * (deg_d[d] + 1))).astype(np.float32)
        norm = (1.0 / (deg_d[:N] + 1)).astype(np.float32)
    g = graph_from_edges(N, Gs, Gd, s, d, w, norm)
    g["planted"] = planted
    return g


def substitute_exact_values(g, seed=0):
    """a partition read from a file (the parts_* goldens) with its own structure and exact values in place of GCN's; the two
    directions are drawn apart (the kernels never relate them)"""
    rng = np.random.default_rng([29, seed])
    h = dict(g)
    h["cscVal"], h["csrVal"] = exact_weights(rng, len(g["rowIdx"])), exact_weights(rng, len(g["colIdx"]))
    h["norm"] = exact_weights(rng, int(g["localVtxCnt"]))
    return h


def side(g, direction):
    """(ptr, idx, val, ghosts) of the adjacency an aggregation walks: the in-edges forward, the out-edges backward"""
    if direction == "bwd":
        return g["rowPtr"], g["colIdx"], g["csrVal"], int(g["dstGhostCnt"])
    return g["colPtr"], g["rowIdx"], g["cscVal"], int(g["srcGhostCnt"])


def features(g, direction, F, exact, seed=0):
    """local rows and ghost rows for one aggregation"""
    N = int(g["localVtxCnt"])
    G = side(g, direction)[3]
    rng = np.random.default_rng([31, seed, N, G, F, int(exact), len(direction)])
    if exact:
        return exact_features(rng, N, F), exact_features(rng, G, F)
    return rng.standard_normal((N, F)).astype(np.float32), rng.standard_normal((G, F)).astype(np.float32)


# ---- the mirror of the dispatch (csrc/abi_stages.hip spmm / spmm_k1s / spmm_k1b / spmm_k1 and what they call) ---------------------------------
def sweep_pick_r(N, group, G, force_r, max_r=10):
    if force_r in (2, 4, 6, 8) or (force_r == 10 and group == 32 and max_r >= 10) or (force_r in (3, 5) and group == 16):
        return force_r
    rpx = (N + 7) // 8
    best, best_fill = 8, 0.0
    for R in PICK_R:
        if (group == 16 and R == 10) or R > max_r:
            continue
        RW = SWEEP_NT // group * R
        tiles = _cdiv(rpx, RW)
        spp = _cdiv(tiles, G)
        fill = rpx / (spp * G * RW) if spp else 0.0
        if fill > best_fill + 0.02:
            best_fill, best = fill, R
    return best


def sweep_rows_for(layout_r, group, G, force_r):
    if force_r and sweep_pick_r(0, group, G, force_r, 10) == force_r:
        return force_r
    return max(2, layout_r // 2) if group == 16 else layout_r


def deal_npos(nl, R, tiles, relief):
    """host/sweep_deal.cpp sweep_deal_plan: the positions of a layout dealt for `tiles` workgroups of 32 lane groups per sweep and XCD"""
    relief = min(relief, R // 2)
    GS, n_x = tiles * 32, (nl + 7) // 8

    def relief_of(rows, lr):
        return (lr * rows + R // 2) // R

    def capacity(need, lr):
        S = _cdiv(need, R)
        last = need - (S - 1) * R
        return (S - 1) * (GS * R - 2 * tiles * relief_of(R, lr)) + GS * last - 2 * tiles * min(relief_of(last, lr), last)

    need0 = max(1, _cdiv(n_x, GS))
    lr = relief
    while True:
        need = need0
        while capacity(need, lr) < n_x:
            need += 1
        if _cdiv(need, R) == _cdiv(need0, R) or lr == 0:
            break
        lr -= 1
    return max(8 * _cdiv(need, R) * GS * R, 8)


def group_step_entries(deg, R):
    """entries per lane group of the one step of a sweep in row order over one source block (spmm_sweep_layout = 0,
    spmm_blk_nb = 1), on a graph without pieces: the sum of the degrees of R consecutive rows"""
    deg = np.asarray(deg, np.int64)
    assert deg.size % (8 * R) == 0                 # (rpx is then a multiple of R: no group straddles two XCDs' ranges)
    return deg.reshape(-1, R).sum(axis=1)


def blk_group_for(opts, ld):
    group = opts["spmm_blk_group"]
    if group not in (8, 16, 32):
        group = 32
    return 16 if ld < 128 and group == 32 else group


def k1_form(ld, slab):
    width = slab if 0 < slab < ld else ld
    ch = (width + 3) // 4
    for lim, G, C in K1_TABLE:
        if lim is None or ch <= lim:
            break
    return G, C, _cdiv(ld // 4, G * C)


class AdjStats:
    """what the mirror needs of one adjacency, computed once: degrees, the rows that read a ghost row, the longest (block, row)
    segment of K1b's layout"""

    def __init__(self, N, ptr, idx):
        self.N = N
        self.ptr, self.idx = np.asarray(ptr, np.int64), np.asarray(idx, np.int64)
        self.deg = np.diff(self.ptr)
        self.nnz = int(self.ptr[-1])
        self.rows = np.repeat(np.arange(N, dtype=np.int64), self.deg)
        self.n_boundary = int(np.unique(self.rows[self.idx >= N]).size) if self.nnz else 0
        self._seg = {}

    def max_segment(self, nb, SB):
        if (nb, SB) not in self._seg:
            self._seg[(nb, SB)] = int(np.bincount(self.rows * nb + self.idx // SB).max()) if self.nnz else 0
        return self._seg[(nb, SB)]


def dispatch(N, ghosts, F, ptr, idx, options=None, static_ghosts=False, unit=False, gnn_gcn=True, cus=CUS_PER_XCD, stats=None):
    """what one aggregation over (ptr, idx) does: the record the coverage assertion and the GPU test's counter check read.
    options: the context's, where they differ from DEFAULTS.  static_ghosts: layer 0's forward aggregation.  unit: the GAT
    prototype's unit-weight form (row_scale)"""
    o = dict(DEFAULTS)
    o.update(options or {})
    st = stats or AdjStats(N, ptr, idx)
    deg, nnz, NG, ld = st.deg, st.nnz, N + ghosts, pad_ld(F)
    G = min(32, cus)
    bf16 = bool(o["gcn_bf16_gather"]) and not unit
    want_nb = o["spmm_blk_nb"]
    group = blk_group_for(o, ld)
    rec = dict(N=N, ghosts=ghosts, F=F, ld=ld, bf16=bf16, unit=unit, options=o)
    layouts = N > 0 and ld >= 32
    has_ghost_rows = ghosts > 0
    force_split = bool(o["spmm_blk_force_split"])
    tiny = not want_nb and NG * group * 16 <= TINY_BYTES

    # K1s
    if layouts and o["spmm_variant"] == 2:
        Rl = sweep_pick_r(N, 32, G, o["spmm_sweep_rows"])
        window_kb = o["spmm_sweep_window_kb"] or (SWEEP_WINDOW_KB_FEW_ROWS if Rl <= 4 else SWEEP_WINDOW_KB)
        window = window_kb << 10
        nb_est = _cdiv(NG * group * 16, window) + 1
        nbx = want_nb or nb_est
        na = tiny or N < 8 or nbx > SWEEP_MAX_NB or nbx * (N + 1) * 8 > OFFSET_TABLE_BYTES
        addr_ok = N * ld * 4 < 2 ** 32 and ghosts * ld * 4 < 2 ** 32 and NG < 2 ** 24
        if not na and group in (16, 32) and addr_ok:
            sd = split_deg(nnz, N)
            pieces = np.where(deg > sd, _cdiv(deg, sd), 1)
            nl = int(pieces.sum())
            # (the layout is built once, with the loader option of that moment: layout_loader, where a walk changed it since)
            relief = LOADER_RELIEF if group == 32 and o.get("layout_loader", o["spmm_sweep_loader"]) else 0
            npos = deal_npos(nl, Rl, G, relief) if o["spmm_sweep_layout"] & 2 else max(_cdiv(nl, Rl) * Rl, 8)
            rb = group * 16
            nbL, nbG = _cdiv(N * rb, window), (_cdiv(ghosts * rb, window) if ghosts else 0)
            if want_nb:
                nbG = max(1, want_nb * ghosts // NG) if ghosts else 0
                nbL = max(1, want_nb - nbG if want_nb > nbG else 1)
            nbL = max(nbL, 1)
            R = sweep_rows_for(Rl, group, G, o["spmm_sweep_rows"])
            RW = SWEEP_NT // group * R
            rpx = _cdiv(_cdiv(npos, 8), R) * R
            tiles_x = _cdiv(rpx, RW)
            slabs = _cdiv(ld // 4, group)
            pair = False if R & 1 else (slabs >= 3 if o["spmm_sweep_pair"] < 0 else o["spmm_sweep_pair"] != 0)
            rec.update(family="k1s", group=group, R=R, layout_R=Rl, forced=bool(o["spmm_sweep_rows"]) and R == o["spmm_sweep_rows"],
                       pair=pair, loader=bool(o["spmm_sweep_loader"]), slabs=slabs, spp=_cdiv(tiles_x, G), ragged=tiles_x % G != 0,
                       pieces=bool((pieces > 1).any()), max_pieces=int(pieces.max()) if N else 0, nb=nbL + nbG, nb_local=nbL,
                       two_launches=has_ghost_rows and 0 < nbL < nbL + nbG, npos=npos, nl=nl, default_window=not want_nb)
            return rec

    # K1b
    if layouts and o["spmm_variant"] >= 1 and not bf16:
        row_bytes = group * 16
        if want_nb:
            nb = _cdiv(want_nb, 8) * 8
        else:
            window = BLOCKED_WINDOW_WIDE if row_bytes >= 512 else BLOCKED_WINDOW_NARROW
            nb = 8
            while _cdiv(NG, nb) * row_bytes > window:
                nb += 8
        if not (tiny or nb > BLOCKED_MAX_NB or nb * (N + 1) * 8 > OFFSET_TABLE_BYTES) and nb * N * ld * 4 <= 48 << 30:
            SB = _cdiv(NG, nb)
            nb_local = min(nb, N // SB)
            max_seg = st.max_segment(nb, SB)
            rec.update(family="k1b", group=group, nb=nb, rounds=nb // 8, nb_local=nb_local,
                       split=force_split and 0 < nb_local < nb, long_segments=max_seg > BLK_SEG_CLAMP, max_segment=max_seg)
            return rec

    # K1
    Gk, Ck, gridy = k1_form(ld, o["spmm_slab"])
    long_rows = bool((deg > LONG_ROW_CLAMP).any())
    skew = N > 0 and int(deg.max()) * N > 8 * nnz + 8 * N
    n_interior = N - st.n_boundary
    rec.update(family="k1", group=Gk, chunks=Ck, gridy=gridy, gridy_by_slab=gridy > 1 and 0 < o["spmm_slab"] < ld,
               order=o["spmm_order"] >= 2 or (o["spmm_order"] == 1 and skew), long_rows=long_rows,
               ragged_rows=N % (4 * (64 // Gk)) != 0, edge_split=None, row_split=False)
    if gnn_gcn and not unit and has_ghost_rows and not long_rows and o["spmm_edge_split"] and not static_ghosts:
        rec["edge_split"] = "one_launch" if not force_split else ("two_launches" if n_interior < N else "two_launches_no_boundary")
    else:
        rec["row_split"] = force_split and has_ghost_rows and 0 < n_interior < N and not long_rows
    return rec


def forms_of(rec):
    """the names of the forms one aggregation reaches (REQUIRED_FORMS lists what the case list has to reach)"""
    f, bf = set(), "+bf16" if rec["bf16"] else ""
    fam = rec["family"]
    if fam == "k1":
        f.add(f"k1:<{rec['group']},{rec['chunks']}>{bf}")
        if rec["gridy"] > 1:
            f.add("k1:gridy_by_slab" + bf if rec["gridy_by_slab"] else "k1:gridy_by_width" + bf)
        f.add(("k1:order" if rec["order"] else "k1:no_order") + bf)
        if rec["long_rows"]:
            f.add("k1:long_rows" + bf)
        if rec["edge_split"]:
            f.add(f"k1:edge_split:{rec['edge_split']}{bf}")
        if rec["row_split"]:
            f.add("k1:row_split" + bf)
        if rec["ragged_rows"]:
            f.add("k1:rows_not_a_multiple_of_the_block" + bf)
    elif fam == "k1b":
        w = "unit" if rec["unit"] else "weighted"
        f |= {f"k1b:group{rec['group']}", "k1b:ghosts" if rec["ghosts"] else "k1b:no_ghosts", f"k1b:{w}",
              "k1b:one_round" if rec["rounds"] == 1 else "k1b:several_rounds"}
        if rec["split"]:
            f.add("k1b:split_launches")
        if rec["long_segments"]:
            f.add("k1b:long_segments")
    else:
        how = "forced" if rec["forced"] else "picked"
        f.add(f"k1s:<{rec['group']},{rec['R']}>:{how}{bf}")
        if not rec["R"] & 1:
            f.add(("k1s:pair" if rec["pair"] else "k1s:no_pair") + bf)
        f.add(("k1s:loader" if rec["loader"] else "k1s:no_loader") + bf)
        f.add("k1s:unit" if rec["unit"] else "k1s:weighted" + bf)
        f.add(("k1s:two_launches" if rec["two_launches"] else "k1s:one_launch") + bf)
        f.add(("k1s:pieces" if rec["pieces"] else "k1s:no_pieces") + bf)
        if rec["max_pieces"] >= 200:
            f.add("k1s:hundreds_of_pieces" + bf)
        f.add(("k1s:one_sweep_per_slab" if rec["spp"] == 1 else "k1s:several_sweeps") + bf)
        if rec["spp"] > 1 and rec["ragged"]:
            f.add("k1s:ragged_last_sweep" + bf)
        if rec["N"] in (8, 9):
            f.add(f"k1s:N={rec['N']}" + bf)
        f.add(("k1s:default_window" if rec["default_window"] else "k1s:explicit_blocks") + bf)
        if rec["nb_local"] == 1 and rec["two_launches"]:
            f.add("k1s:nb_local=1" + bf)
        if rec["two_launches"] and rec["nb"] - rec["nb_local"] == 1:
            f.add("k1s:one_ghost_block" + bf)
    return f


def _with_bf16(names):
    return names + [n + "+bf16" for n in names]


REQUIRED_FORMS = (
    _with_bf16([f"k1:<{g},{c}>" for g, c in K1_FORMS] +
               ["k1:gridy_by_width", "k1:gridy_by_slab", "k1:order", "k1:no_order", "k1:long_rows", "k1:edge_split:one_launch",
                "k1:edge_split:two_launches", "k1:edge_split:two_launches_no_boundary", "k1:row_split",
                "k1:rows_not_a_multiple_of_the_block"]) +
    ["k1b:group8", "k1b:group16", "k1b:group32", "k1b:ghosts", "k1b:no_ghosts", "k1b:unit", "k1b:weighted", "k1b:one_round",
     "k1b:several_rounds", "k1b:split_launches", "k1b:long_segments"] +
    _with_bf16([f"k1s:<32,{r}>:picked" for r in (2, 4, 6, 8, 10)] + [f"k1s:<16,{r}>:picked" for r in (2, 3, 4, 5)] +
               [f"k1s:<16,{r}>:forced" for r in (6, 8)] +
               ["k1s:pair", "k1s:no_pair", "k1s:loader", "k1s:no_loader", "k1s:weighted", "k1s:one_launch", "k1s:two_launches",
                "k1s:pieces", "k1s:no_pieces", "k1s:hundreds_of_pieces", "k1s:one_sweep_per_slab", "k1s:several_sweeps",
                "k1s:ragged_last_sweep", "k1s:N=8", "k1s:N=9", "k1s:default_window", "k1s:explicit_blocks",
                "k1s:nb_local=1", "k1s:one_ghost_block"]) +
    ["k1s:unit"])

# forms the dispatch cannot reach, each with the reason
UNREACHABLE_FORMS = {
    "k1s:<16,6>:picked": "sweep_rows_for halves the layout's rows for 16-lane launches and sweep_pick_r deals at most ten: 5 is the most",
    "k1s:<16,8>:picked": "as <16,6>: eight rows on 16 lanes only when option spmm_sweep_rows forces them",
    "k1s:npos_padded_to_8": "npos is raised to 8 only for fewer than 8 positions, i.e. fewer than 8 rows, and ensure_sweep / sweep_supported "
                            "hand N < 8 to the next family (case n7 runs it: K1b); N = 8 and 9 are in the list",
    "k1s:unit+bf16": "the bf16 rows are GCN's (spmm() refuses row_scale with bf16)",
    "k1b:*+bf16": "K1b has no bf16 form: the bf16 dispatch takes K1 instead, an explicit spmm_variant = 1 is refused",
}


# ---- the case list ------------------------------------------------------------------------------------------------------------------------
# (id, graph, F, options set before the graph is uploaded).  Every case runs with spmm_variant 0, 1 and 2 and in every direction
# (CASE_DIRECTIONS); the walk of the schedules inside a case is WALK.
CASES = [
    # K1's eight forms and both kinds of grid.y on a graph with multi-edges and self loops; 5 003 rows: no multiple of any block
    ("multi_F20", "multi:5003:60000", 20, {}), ("multi_F41", "multi:5003:60000", 41, {}), ("multi_F100", "multi:5003:60000", 100, {}),
    ("multi_F200", "multi:5003:60000", 200, {}), ("multi_F300", "multi:5003:60000", 300, {}), ("multi_F500", "multi:5003:60000", 500, {}),
    ("multi_F602", "multi:5003:60000", 602, {}), ("multi_F1433", "multi:5003:60000", 1433, {}),
    ("multi_F602_slab64", "multi:5003:60000", 602, {"spmm_slab": 64}),
    # the same graph through the layouts: explicit block counts (the graph is L2-sized)
    ("multi_F128_nb8", "multi:5003:60000", 128, {"spmm_blk_nb": 8}), ("multi_F64_nb24_g8", "multi:5003:60000", 64, {"spmm_blk_nb": 24, "spmm_blk_group": 8}),
    ("multi_F602_nb16", "multi:5003:60000", 602, {"spmm_blk_nb": 16}),
    # rows per lane group by sweep_pick_r alone: 2 / 4 / 6 / 8 / 10 on 32 lanes (F = 128), 2 / 2 / 3 / 4 / 5 on 16 (F = 64)
    ("u1025_F128", "uniform:1025:12000", 128, {"spmm_blk_nb": 8}), ("u1025_F64", "uniform:1025:12000", 64, {"spmm_blk_nb": 8}),
    ("u20k_F128", "uniform:20000:240000", 128, {}), ("u20k_F64", "uniform:20000:240000", 64, {}),
    ("u33k_F128", "uniform:33000:400000", 128, {}), ("u33k_F64", "uniform:33000:400000", 64, {}),
    ("u120k_F128", "uniform:120000:1400000", 128, {}), ("u120k_F64", "uniform:120000:1400000", 64, {}),
    ("u70001_F128", "uniform:70001:800000", 128, {}), ("u70001_F64", "uniform:70001:800000", 64, {}),
    # forced rows: six and eight on 16 lanes; two rows on a large graph and three on a layout dealt for eight (several sweeps
    # per slab, a ragged last one); K1b's order instead of the deal (spmm_sweep_layout = 0: ragged by itself)
    ("u33k_F64_r6", "uniform:33000:400000", 64, {"spmm_sweep_rows": 6}), ("u33k_F64_r8", "uniform:33000:400000", 64, {"spmm_sweep_rows": 8}),
    ("u70001_F128_r2", "uniform:70001:800000", 128, {"spmm_sweep_rows": 2}), ("u120k_F64_r3", "uniform:120000:1400000", 64, {"spmm_sweep_rows": 3}),
    ("u33k_F256_layout0", "uniform:33000:400000", 256, {"spmm_sweep_layout": 0}),
    # one lane group's entries of one step on both sides of a staging pass
    ("staging_F128", "staging", 128, {"spmm_sweep_layout": 0, "spmm_blk_nb": 1, "spmm_sweep_rows": 4}),
    ("staging_F64", "staging", 64, {"spmm_sweep_layout": 0, "spmm_blk_nb": 1, "spmm_sweep_rows": 4}),
    # tiny partitions of the sweep: N = 8, 9 (and 7, which the sweep refuses), positions padded up to 8
    ("n7", "uniform:7:30", 128, {"spmm_blk_nb": 8}), ("n8", "uniform:8:40", 128, {"spmm_blk_nb": 8}), ("n9", "uniform:9:40", 64, {"spmm_blk_nb": 8}),
    # skew: pieces, long segments, long rows
    ("powerlaw_F128", "powerlaw:30000:500000", 128, {}), ("powerlaw_F602", "powerlaw:30000:500000", 602, {}),
    ("planted_F128", "planted", 128, {}), ("planted_F64", "planted", 64, {}), ("planted_F300_g16", "planted", 300, {"spmm_blk_group": 16}),
    ("hubs_F128", "hubs", 128, {"spmm_blk_nb": 8}), ("hubs_F41", "hubs", 41, {"spmm_blk_nb": 16}), ("hubs_F602", "hubs", 602, {"spmm_blk_nb": 8}),
    # partitions with ghost rows: a small share (one ghost block), more ghosts than local rows, one local block, ghost rows
    # that no edge of one side reads (no boundary rows there)
    ("ghosts_small_F128", "ghosts:30000:2000:2500:360000:20000:25000", 128, {}),
    ("ghosts_small_F64", "ghosts:30000:2000:2500:360000:20000:25000", 64, {}),
    ("ghosts_small_F128_nb2", "ghosts:30000:2000:2500:360000:20000:25000", 128, {"spmm_blk_nb": 2}),
    ("ghosts_big_F128", "ghosts:20000:30000:26000:150000:300000:280000", 128, {}),
    ("ghosts_big_F602", "ghosts:20000:30000:26000:150000:300000:280000", 602, {}),
    ("ghosts_big_F300_nb24", "ghosts:20000:30000:26000:150000:300000:280000", 300, {"spmm_blk_nb": 24}),
    ("ghosts_unread_F128", "ghosts:16000:50:40:200000:0:0", 128, {}),
]
CASE_IDS = [c[0] for c in CASES]
FAMILIES = {"k1": 0, "k1b": 1, "k1s": 2}          # family asked for -> spmm_variant (the mirror says which one runs)
# fwd0: layer 0's forward aggregation ("x", "fg"@0 -> "ah"@0: ghost rows that never travel); fwd1: layer 1's ("h"@0, "fg"@1 ->
# "ah"@1); bwd: layer 1's backward ("grad"@1, "bg"@0 -> "aTg"@0)
DIRECTIONS = ["fwd0", "fwd1", "bwd"]

# the schedules walked inside one case: none may change a bit.  (option, values); the first value is the state the others return to
WALK = [("spmm_blk_force_split", (0, 1)), ("spmm_order", (1, 0, 2)), ("spmm_edge_split", (1, 0)), ("spmm_sweep_pair", (-1, 0, 1)),
        ("spmm_sweep_loader", (1, 0)), ("gcn_bf16_gather", (0, 1, 2))]


def walk_settings(family):
    """the option settings one test walks: the base, then every option of WALK on its own, then force_split together with the
    others that change what a split launch does"""
    out = [{}]
    for key, vals in WALK:
        if key == "gcn_bf16_gather" and family == "k1b":
            continue                              # (refused with spmm_variant = 1)
        out += [{key: v} for v in vals[1:]]
    out += [{"spmm_blk_force_split": 1, "spmm_order": 2}, {"spmm_blk_force_split": 1, "spmm_edge_split": 0}]
    if family != "k1b":
        out += [{"spmm_blk_force_split": 1, "gcn_bf16_gather": 2}, {"spmm_sweep_pair": 1, "spmm_sweep_loader": 0, "gcn_bf16_gather": 2},
                {"spmm_sweep_pair": 0, "gcn_bf16_gather": 2}, {"spmm_order": 0, "gcn_bf16_gather": 2}, {"spmm_order": 2, "gcn_bf16_gather": 2}]
    return out


def bf16_on(options, direction):
    m = options.get("gcn_bf16_gather", 0)
    return m >= 2 if direction == "bwd" else m >= 1


@functools.lru_cache(maxsize=8)
def _stats(gname, direction):
    g = graph(gname)
    ptr, idx, _, _ = side(g, direction)
    return AdjStats(int(g["localVtxCnt"]), ptr, idx)


def case_record(case, family, direction, extra=None):
    """the mirror's record of one aggregation of a case"""
    _, gname, F, opts = case
    g = graph(gname)
    ptr, idx, _, ghosts = side(g, direction)
    o = dict(opts)
    o["layout_loader"] = opts.get("spmm_sweep_loader", DEFAULTS["spmm_sweep_loader"])
    o["spmm_variant"] = FAMILIES[family]
    o.update(extra or {})
    o["gcn_bf16_gather"] = int(bf16_on(o, direction))
    return dispatch(int(g["localVtxCnt"]), ghosts, F, ptr, idx, o, static_ghosts=direction == "fwd0",
                    stats=_stats(gname, "bwd" if direction == "bwd" else "fwd"))


# the unit-weight form (the GAT prototype's neighbour sum): (id, graph, F, options)
UNIT_CASES = [
    ("unit_sweep_u20k_F128", "uniform:20000:240000", 128, {}),
    ("unit_sweep_ghosts_F64", "ghosts:30000:2000:2500:360000:20000:25000", 64, {}),
    ("unit_sweep_planted_F128", "planted", 128, {}),
    ("unit_blocked_u20k_F128", "uniform:20000:240000", 128, {"spmm_variant": 1}),
    ("unit_blocked_ghosts_F64", "ghosts:30000:2000:2500:360000:20000:25000", 64, {"spmm_variant": 1, "spmm_blk_nb": 16}),
    ("unit_blocked_planted_F41_g8", "planted", 41, {"spmm_variant": 1, "spmm_blk_group": 8, "spmm_blk_nb": 8}),   # (128-byte slabs: L2-sized without a count)
]
UNIT_CASE_IDS = [c[0] for c in UNIT_CASES]


def unit_record(case):
    _, gname, F, opts = case
    g = graph(gname)
    ptr, idx, _, ghosts = side(g, "fwd0")
    return dispatch(int(g["localVtxCnt"]), ghosts, F, ptr, idx, opts, unit=True, gnn_gcn=False, stats=_stats(gname, "fwd"))


def covered_forms():
    """every form the GPU case list reaches, by the mirror"""
    got = set()
    for case in CASES:
        for family in FAMILIES:
            for direction in DIRECTIONS:
                for extra in walk_settings(family):
                    got |= forms_of(case_record(case, family, direction, extra))
    for case in UNIT_CASES:
        got |= forms_of(unit_record(case))
    return got
