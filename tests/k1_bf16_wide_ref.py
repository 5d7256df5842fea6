"""What the tests of K1's wide bf16 row gather (dory_k1_bf16_wide; csrc/spmm.hip: spmm_rows_bf16x8_kernel) share: a Python mirror of
the form rule (csrc/k1_shapes.hpp: k1_rows8_form), the widths the GPU test runs with the form each must take, and the two hand-built
graphs -- small enough that a context costs nothing, with a degree planted at every point where the kernel's loops change shape.

tests/test_k1_bf16_wide_form.py holds the mirror against the library and the graphs against their own description, without a GPU;
tests/test_gpu_k1_bf16_wide.py runs them."""
import functools

import numpy as np

import aggregate_ref as ar

# ---- the rule -------------------------------------------------------------------------------------------------------------------
WIDE_TABLE = [(8, 8, 1), (16, 16, 1), (32, 32, 1), (64, 64, 1), (96, 32, 3), (128, 64, 2), (None, 64, 3)]   # ch8 <=, lanes, chunks
WIDE_FORMS = sorted({(g, c) for _, g, c in WIDE_TABLE})


def form(ld, slab=0):
    """None where K1 has no wide form for rows of ld floats under spmm_slab = slab, else (lanes, chunks, gridDim.y)"""
    if ld < 64 or ld % 8:
        return None
    width = slab if 0 < slab < ld else ld
    if width < 64:
        return None
    ch8 = (width + 7) // 8
    for lim, g, c in WIDE_TABLE:
        if lim is None or ch8 <= lim:
            break
    return g, c, -(-(ld // 8) // (g * c))


# (F, spmm_slab) -> the form: one width per instantiation, the edges of the rule, both kinds of gridDim.y, the two fall-backs
WIDTHS = [
    (41, 0, (8, 1, 1)), (100, 0, (16, 1, 1)), (200, 0, (32, 1, 1)), (300, 0, (64, 1, 1)), (500, 0, (64, 1, 1)),
    (602, 0, (32, 3, 1)),        # ld 608: 76 of 96 lane-chunks
    (1000, 0, (64, 2, 1)), (1433, 0, (64, 3, 1)),
    (1600, 0, (64, 3, 2)),       # past 1536 floats: gridDim.y = 2 by width
    (602, 64, (8, 1, 10)),       # gridDim.y = 10 by slab
    (20, 0, None), (100, 32, None),   # ld 32; passes of 32 floats: narrow, counted
]

# ---- the graphs -----------------------------------------------------------------------------------------------------------------
N_ROWS, N_SRC_GHOSTS, N_DST_GHOSTS = 203, 37, 29      # 203: no multiple of 4 .. 32, the rows of a block for any lane group
PLANTED = ar.PLANTED_SHORT                            # 0, 1, 3, 4, 5 and g - 1, g, g + 1 for the lane groups; 126 .. 129
LONG_ROW = ar.LONG_ROW_CLAMP + ar.LONG_ROW_CHUNK + 3  # K1's clamped launch, one whole chunk and a chunk of three entries
P_LOCAL, P_GHOSTS = 150, 90


def _values(values, rng, s, d, N, Gs, Gd):
    if values == "exact":
        return ar.exact_weights(rng, s.size), ar.exact_weights(rng, N)
    deg_d = np.concatenate([np.bincount(d[d < N], minlength=N), rng.integers(1, 60, Gd)]).astype(np.float64)
    deg_s = np.concatenate([deg_d[:N], rng.integers(1, 60, Gs)])
    return (1.0 / np.sqrt((deg_s[s] + 1) * (deg_d[d] + 1))).astype(np.float32), (1.0 / (deg_d[:N] + 1)).astype(np.float32)


@functools.lru_cache(maxsize=8)
def graph203(values="exact", long_row=False):
    """203 local rows, 37 source-side and 29 destination-side ghost rows.  Vertices [0, n) have the in-degrees of PLANTED, vertices
    [n, 2n) its out-degrees, their neighbours drawn from the other local vertices and the ghosts; the others are joined by random
    edges of which half are repeated once or twice (multi-edges, not adjacent) with a self loop on every third.  long_row: vertex
    2n has LONG_ROW in-edges and vertex 2n + 1 LONG_ROW out-edges over the same few hundred neighbours on top"""
    rng = np.random.default_rng([61, int(long_row)])
    N, Gs, Gd, n = N_ROWS, N_SRC_GHOSTS, N_DST_GHOSTS, len(PLANTED)
    free = np.arange(2 * n + 2, N)          # (2n, 2n + 1: the long rows' vertices, without an edge otherwise)
    s0, d0 = free[rng.integers(0, free.size, 900)], free[rng.integers(0, free.size, 900)]
    loops = free[::3]
    s = [s0, s0[:450], s0[:200], loops, N + rng.integers(0, Gs, 160), free[rng.integers(0, free.size, 140)]]
    d = [d0, d0[:450], d0[:200], loops, free[rng.integers(0, free.size, 160)], N + rng.integers(0, Gd, 140)]
    rows = np.repeat(np.arange(n), PLANTED)
    src_pool, dst_pool = np.concatenate([free, N + np.arange(Gs)]), np.concatenate([free, N + np.arange(Gd)])
    s += [src_pool[rng.integers(0, src_pool.size, rows.size)], rows + n]
    d += [rows, dst_pool[rng.integers(0, dst_pool.size, rows.size)]]
    if long_row:
        s += [src_pool[rng.integers(0, src_pool.size, LONG_ROW)], np.full(LONG_ROW, 2 * n + 1)]
        d += [np.full(LONG_ROW, 2 * n), dst_pool[rng.integers(0, dst_pool.size, LONG_ROW)]]
    s, d = np.concatenate(s), np.concatenate(d)
    o = rng.permutation(s.size)
    s, d = s[o], d[o]
    w, norm = _values(values, rng, s, d, N, Gs, Gd)
    g = ar.graph_from_edges(N, Gs, Gd, s, d, w, norm)
    g["planted"] = {"in": dict(enumerate(PLANTED)), "out": {n + i: dg for i, dg in enumerate(PLANTED)}}
    return g


@functools.lru_cache(maxsize=4)
def partition150(values="exact"):
    """150 local rows with 90 ghost rows on either side.  In-edges: rows [0, 40) have ghost sources only, [40, 80) local sources only,
    the rest both.  Out-edges: no edge reaches a destination-side ghost -- the side whose ghosts nothing reads (no boundary rows)"""
    rng = np.random.default_rng(67)
    N, G = P_LOCAL, P_GHOSTS
    ls, ld = rng.integers(0, N, 1400), rng.integers(40, N, 1400)
    gs, gd = N + rng.integers(0, G, 700), np.concatenate([rng.integers(0, 40, 250), rng.integers(80, N, 450)])
    s, d = np.concatenate([ls, gs]), np.concatenate([ld, gd])
    o = rng.permutation(s.size)
    s, d = s[o], d[o]
    w, norm = _values(values, rng, s, d, N, G, G)
    return ar.graph_from_edges(N, G, G, s, d, w, norm)
