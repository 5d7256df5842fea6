"""dory_row_edge_split_plan (include/dorylus_host.h; host/row_chunks.cpp): every row's entries regrouped local ids first -- the copy
dory_gatmh_row_gather_edge_split builds per adjacency for the carry kernels of the multi-head GAT's row-gather family -- against a
numpy stable partition.  Pure host code: no GPU."""
import ctypes as C
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _want(ptr, idx, N):
    """the definition, row by row: the ids < N in their order, then the ids >= N in their order; mid = where the second run starts"""
    ptr = np.asarray(ptr, np.int64)
    idx = np.asarray(idx, np.uint32)
    out, mid = np.zeros_like(idx), np.zeros(ptr.size - 1, np.uint64)
    for v in range(ptr.size - 1):
        row = idx[ptr[v]:ptr[v + 1]]
        ghost = row >= N
        order = np.argsort(ghost, kind="stable")          # False (local) before True (ghost), ties in original order
        out[ptr[v]:ptr[v + 1]] = row[order]
        mid[v] = ptr[v] + int(np.count_nonzero(~ghost))
    return out, mid


def _check(da, ptr, idx, N, what):
    ptr, idx = np.asarray(ptr, np.uint64), np.asarray(idx, np.uint32)
    keep_ptr, keep_idx = ptr.copy(), idx.copy()
    out, mid = da.row_edge_split_plan(ptr, idx, N)
    assert np.array_equal(ptr, keep_ptr) and np.array_equal(idx, keep_idx), what          # the inputs are not touched
    wo, wm = _want(ptr, idx, N)
    assert out.dtype == np.uint32 and mid.dtype == np.uint64, what
    assert np.array_equal(out, wo), (what, out, wo)
    assert np.array_equal(mid, wm), (what, mid, wm)
    p = ptr.astype(np.int64)
    for v in range(p.size - 1):
        a, b, m = p[v], p[v + 1], int(mid[v])
        assert a <= m <= b, (what, v)
        assert np.all(out[a:m] < N) and np.all(out[m:b] >= N), (what, v)
        assert np.array_equal(np.sort(out[a:b]), np.sort(idx[a:b])), (what, v)            # a permutation of the row's ids
    return out, mid


def _csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    idx = np.array([x for r in rows for x in r], np.uint32)
    return ptr, idx


def test_rows_of_every_kind(da):
    N = 6
    rows = [[],                                # no entries: mid = ptr[v] = ptr[v + 1]
            [3, 0, 5, 3],                      # all local: unchanged, mid = ptr[v + 1]
            [N + 4, N, N + 2],                 # all ghost: unchanged, mid = ptr[v]
            [N + 1, 1, N, 0, N + 3, 2],        # alternating, ghost first
            [4, N + 9, 5, N + 8, 4, N + 9],    # alternating, local first, repeated ids
            [N - 1, N]]                        # the edge of the local range
    ptr, idx = _csr(rows)
    out, mid = _check(da, ptr, idx, N, "every kind")
    assert out.tolist() == [3, 0, 5, 3, N + 4, N, N + 2, 1, 0, 2, N + 1, N, N + 3, 4, 5, 4, N + 9, N + 8, N + 9, N - 1, N]
    assert mid.tolist() == [0, 4, 4, 10, 16, 20]


def test_no_local_vertices(da):
    ptr, idx = _csr([[2, 0, 1], [], [7]])
    out, mid = _check(da, ptr, idx, 0, "N = 0")                  # every id is a ghost id: nothing moves
    assert np.array_equal(out, idx) and mid.tolist() == [0, 3, 3]
    out, mid = da.row_edge_split_plan(np.zeros(1, np.uint64), np.zeros(0, np.uint32), 0)      # and no rows at all
    assert out.size == 0 and mid.size == 0


def test_random_adjacencies(da):
    rng = np.random.default_rng(31)
    for N, G, E in ((1, 0, 0), (1, 1, 3), (33, 5, 200), (257, 40, 900), (500, 1, 2000), (64, 64, 5000)):
        deg = rng.multinomial(E, np.ones(N) / N)
        ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
        idx = rng.integers(0, N + G, E).astype(np.uint32)
        _check(da, ptr, idx, N, (N, G, E))


def test_pointer_values_past_32_bits(da):
    """positions are 64-bit: an adjacency whose offsets start past 2^32 (the arrays handed over as if they began at entry 0)"""
    lib = da.load()
    base = (1 << 32) + 5
    rows = [[9, 1, 8, 0], [], [7, 7, 2], [3]]
    N = 4
    rel, idx = _csr(rows)
    ptr = rel + np.uint64(base)
    out, mid = np.full(idx.size, 0xFFFFFFFF, np.uint32), np.zeros(len(rows), np.uint64)
    rc = lib.dory_row_edge_split_plan(ptr.ctypes.data_as(C.c_void_p), C.c_void_p(idx.ctypes.data - 4 * base), len(rows), N,
                                      C.c_void_p(out.ctypes.data - 4 * base), mid.ctypes.data_as(C.c_void_p))
    assert rc == 0
    wo, wm = _want(rel, idx, N)
    assert np.array_equal(out, wo)
    assert np.array_equal(mid, wm + np.uint64(base)) and int(mid[0]) > (1 << 32)


def test_committed_partitions_both_adjacencies_every_rank(da):
    import partition_oracle as po
    cases = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "parts_*")))
    assert cases
    moved = 0
    for case in cases:
        bins = sorted(glob.glob(os.path.join(case, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
        assert bins, case
        for b in bins:
            g = po.parse_graph_bin(open(b, "rb").read())
            N = int(g["localVtxCnt"])
            for pk, ik in (("colPtr", "rowIdx"), ("rowPtr", "colIdx")):
                out, _ = _check(da, g[pk], g[ik], N, (os.path.basename(case), os.path.basename(b), pk))
                moved += int(not np.array_equal(out, np.asarray(g[ik], np.uint32)))
    assert moved       # (the fixtures hold ranks whose rows mix local and ghost ids)


def test_bad_input_is_refused(da):
    lib = da.load()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    idx, out, mid = np.zeros(4, np.uint32), np.zeros(4, np.uint32), np.zeros(2, np.uint64)
    ok, dec = np.array([0, 2, 4], np.uint64), np.array([0, 3, 2], np.uint64)
    assert lib.dory_row_edge_split_plan(None, vp(idx), 2, 2, vp(out), vp(mid)) != 0
    assert lib.dory_row_edge_split_plan(vp(dec), vp(idx), 2, 2, vp(out), vp(mid)) != 0
    assert lib.dory_row_edge_split_plan(vp(ok), None, 2, 2, vp(out), vp(mid)) != 0            # entries, no idx
    assert lib.dory_row_edge_split_plan(vp(ok), vp(idx), 2, 2, None, vp(mid)) != 0
    assert lib.dory_row_edge_split_plan(vp(ok), vp(idx), 2, 2, vp(idx), vp(mid)) != 0         # in place
    assert lib.dory_row_edge_split_plan(vp(ok), vp(idx), 2, 2, vp(out), None) != 0
    assert lib.dory_row_edge_split_plan(vp(ok), vp(idx), 2, 2, vp(out), vp(mid)) == 0
    with pytest.raises(da.DoryError):
        da.row_edge_split_plan(dec, idx, 2)
    with pytest.raises(da.DoryError):
        da.row_edge_split_plan(np.array([0, 2, 9], np.uint64), idx, 2)       # ptr names more entries than idx has


def test_entry_points_are_exported_and_bound(da):
    lib = da.load()
    for name in ("dory_row_edge_split_plan", "dory_gatmh_row_gather_edge_split", "dory_gatmh_row_gather_edge_split_stats"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "dory_gatmh_row_gather_edge_split" in da.SYMBOLS and "dory_gatmh_row_gather_edge_split_stats" in da.SYMBOLS
    assert callable(da.row_edge_split_plan)
    assert callable(da.Context.gatmh_row_gather_edge_split) and callable(da.Context.gatmh_row_gather_edge_split_stats)
    assert len(da.Context.GATMH_ROWS_EDGE_SPLIT_STATS) == 8


def test_null_context_fails(da):
    lib = da.load()
    assert lib.dory_gatmh_row_gather_edge_split(None, 1) != 0
    v = [C.c_uint64(0) for _ in range(8)]
    assert lib.dory_gatmh_row_gather_edge_split_stats(None, *[C.byref(x) for x in v]) != 0
