"""dory_row_interior_plan (include/dorylus_host.h; host/row_chunks.cpp): the rows of a partition's adjacency that read no ghost row
-- the plan dory_gatmh_row_gather_overlap builds for the multi-head GAT's row-gather kernels -- against a numpy restatement.  Pure
host code: no GPU."""
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
    """the definition: boundary = a row with an entry >= N; interior = every other row (a row without entries too)"""
    ghost = np.zeros(N, bool)
    ghost[np.repeat(np.arange(N), np.diff(np.asarray(ptr, np.int64)))[np.asarray(idx, np.int64) >= N]] = True
    return np.flatnonzero(~ghost), np.flatnonzero(ghost)


def _check(da, ptr, idx, N, what):
    inter, bound = da.row_interior_plan(ptr, idx, N)
    wi, wb = _want(ptr, idx, N)
    assert inter.dtype == bound.dtype == np.uint32, what
    assert np.array_equal(inter, wi), (what, inter, wi)
    assert np.array_equal(bound, wb), (what, bound, wb)
    # ascending, disjoint, together [0, N)
    assert np.all(np.diff(inter.astype(np.int64)) > 0) and np.all(np.diff(bound.astype(np.int64)) > 0), what
    assert np.array_equal(np.sort(np.concatenate([inter, bound])), np.arange(N)), what
    return inter, bound


def _csr(rows):
    ptr = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.uint64)
    idx = np.array([x for r in rows for x in r], np.uint32)
    return ptr, idx


def test_no_rows(da):
    inter, bound = _check(da, np.zeros(1, np.uint64), np.zeros(0, np.uint32), 0, "N = 0")
    assert inter.size == 0 and bound.size == 0


def test_adjacency_without_entries_is_all_interior(da):
    inter, bound = _check(da, np.zeros(8, np.uint64), np.zeros(0, np.uint32), 7, "no entries")
    assert inter.size == 7 and bound.size == 0


def test_rows_at_the_edge_of_the_local_range(da):
    N = 6
    rows = [[N - 1],                 # the largest local id: interior
            [N],                     # the first ghost id: boundary
            [N, N + 3, N + 1],       # ghost ids only
            [2, 2, 2, 2],            # repeated local ids: interior
            [N + 2, N + 2, 1, 1],    # repeated ids, ghost ones among them: boundary
            []]                      # no entries: interior (its only edge is the self edge)
    ptr, idx = _csr(rows)
    inter, bound = _check(da, ptr, idx, N, "edge rows")
    assert inter.tolist() == [0, 3, 5] and bound.tolist() == [1, 2, 4]


def test_random_adjacencies(da):
    rng = np.random.default_rng(3)
    for N, G, E in ((1, 0, 0), (1, 1, 3), (33, 5, 200), (257, 40, 900), (500, 1, 2000)):
        deg = rng.multinomial(E, np.ones(N) / N)
        ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
        idx = rng.integers(0, N + G, E).astype(np.uint32)
        _check(da, ptr, idx, N, (N, G, E))


def test_committed_partitions_both_adjacencies_every_rank(da):
    import partition_oracle as po
    cases = sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "parts_*")))
    assert cases
    seen_both = 0
    for case in cases:
        bins = sorted(glob.glob(os.path.join(case, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
        assert bins, case
        for b in bins:
            g = po.parse_graph_bin(open(b, "rb").read())
            N = int(g["localVtxCnt"])
            for pk, ik in (("colPtr", "rowIdx"), ("rowPtr", "colIdx")):
                inter, bound = _check(da, g[pk], g[ik], N, (os.path.basename(case), os.path.basename(b), pk))
                seen_both += bool(inter.size and bound.size)
    assert seen_both       # (the fixtures hold ranks with rows of both kinds)


def test_bad_input_is_refused(da):
    lib = da.load()
    ni, nb = C.c_uint32(), C.c_uint32()
    idx = np.zeros(4, np.uint32)
    assert lib.dory_row_interior_plan(None, idx.ctypes.data_as(C.c_void_p), 2, C.byref(ni), C.byref(nb), None, None) != 0
    dec = np.array([0, 3, 2], np.uint64)
    assert lib.dory_row_interior_plan(dec.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 2, C.byref(ni), C.byref(nb), None, None) != 0
    ok = np.array([0, 2, 4], np.uint64)
    assert lib.dory_row_interior_plan(ok.ctypes.data_as(C.c_void_p), None, 2, C.byref(ni), C.byref(nb), None, None) != 0     # entries, no idx
    assert lib.dory_row_interior_plan(ok.ctypes.data_as(C.c_void_p), idx.ctypes.data_as(C.c_void_p), 2, C.byref(ni), C.byref(nb), None, None) == 0
    assert (ni.value, nb.value) == (2, 0)
    with pytest.raises(da.DoryError):
        da.row_interior_plan(dec, idx, 2)
    with pytest.raises(da.DoryError):
        da.row_interior_plan(ok, idx, 3)       # ptr does not have N + 1 entries


def test_entry_points_are_exported_and_bound(da):
    lib = da.load()
    for name in ("dory_row_interior_plan", "dory_gatmh_row_gather_overlap", "dory_gatmh_row_gather_overlap_stats"):
        assert hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert "dory_gatmh_row_gather_overlap" in da.SYMBOLS and "dory_gatmh_row_gather_overlap_stats" in da.SYMBOLS
    assert callable(da.row_interior_plan)
    assert callable(da.Context.gatmh_row_gather_overlap) and callable(da.Context.gatmh_row_gather_overlap_stats)
    assert len(da.Context.GATMH_ROWS_OVERLAP_STATS) == 7


def test_null_context_fails(da):
    lib = da.load()
    assert lib.dory_gatmh_row_gather_overlap(None, 1) != 0
    v = [C.c_uint64(0) for _ in range(7)]
    assert lib.dory_gatmh_row_gather_overlap_stats(None, *[C.byref(x) for x in v]) != 0
