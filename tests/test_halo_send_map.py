"""dory_halo_send_map (include/dorylus_host.h; host/partition.cpp): the send lists of a halo plan turned round, row -> slots of the
packed send buffer -- what the GEMM epilogues of the fused halo pack (dory_halo_fused_pack) index by.  Pure host code: against a
numpy inverse on hand-made plans and on the send lists of the golden partitions.  No GPU needed."""
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def inverse(N, lists):
    """the definition: slot s of the concatenated lists carries row flat[s]; a row's slots in ascending order"""
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])
    order = np.argsort(flat, kind="stable")            # stable: equal rows keep their slot order
    ptr = np.zeros(N + 1, np.int64)
    np.add.at(ptr, flat + 1, 1)
    return np.cumsum(ptr).astype(np.uint32), order.astype(np.uint32)


def check(da, N, lists):
    row_ptr, row_slots = da.halo_send_map(N, lists)
    want_ptr, want_slots = inverse(N, lists)
    assert row_ptr.dtype == np.uint32 and row_ptr.shape == (N + 1,)
    assert np.array_equal(row_ptr, want_ptr)
    assert np.array_equal(row_slots, want_slots)
    total = sum(len(x) for x in lists)
    assert row_ptr[0] == 0 and row_ptr[N] == total
    assert sorted(row_slots.tolist()) == list(range(total))                      # every slot exactly once
    flat = np.concatenate([np.asarray(x, np.int64) for x in lists] + [np.zeros(0, np.int64)])
    for r in range(N):
        mine = row_slots[row_ptr[r]:row_ptr[r + 1]]
        assert np.all(np.diff(mine.astype(np.int64)) > 0)                        # a row's slots ascend
        assert np.all(flat[mine] == r)
    return row_ptr, row_slots


def test_rows_in_no_one_and_all_lists(da):
    # P = 4, this rank is 0 (its own list is empty): row 5 goes nowhere, row 0 to one peer, row 3 to every peer
    lists = [[], [3, 0, 7], [7, 3], [3, 9, 8]]
    row_ptr, row_slots = check(da, 10, lists)
    deg = np.diff(row_ptr.astype(np.int64))
    assert deg[5] == 0 and deg[0] == 1 and deg[3] == 3 and deg.max() == 3      # at most num_nodes - 1 slots
    assert row_slots[row_ptr[3]:row_ptr[4]].tolist() == [0, 4, 5]


def test_unsorted_lists_and_an_empty_peer(da):
    check(da, 12, [[11, 2, 5, 0], [], [5, 11], [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11][::-1]])


def test_empty_plan_and_single_row(da):
    row_ptr, row_slots = check(da, 6, [[], [], []])
    assert not row_ptr.any() and row_slots.size == 0
    check(da, 1, [[], [0], [0]])
    check(da, 1, [[], []])
    check(da, 0, [[], []])


def test_a_row_listed_twice_gets_two_slots(da):
    row_ptr, row_slots = check(da, 5, [[], [4, 2, 4], [4]])
    assert row_slots[row_ptr[4]:row_ptr[5]].tolist() == [0, 2, 3]


def test_an_id_out_of_range_is_refused(da):
    with pytest.raises(da.DoryError, match="out of range"):
        da.halo_send_map(5, [[], [1, 5]])
    with pytest.raises(da.DoryError, match="out of range"):
        da.halo_send_map(0, [[], [0]])


def test_random_plans(da):
    rng = np.random.default_rng(3)
    for N, P in ((1, 2), (31, 4), (300, 8), (1000, 16)):
        lists = [rng.integers(0, N, rng.integers(0, 2 * N)).tolist() if q else [] for q in range(P)]
        check(da, N, lists)


@pytest.mark.parametrize("case", sorted(os.path.basename(d) for d in glob.glob(os.path.join(ROOT, "tests", "golden", "parts_*"))))
def test_golden_plans(da, case):
    """the send lists the reference's partitioner wrote into graph.<id>.bin, both directions of every rank; and the plan is
    consistent across ranks: what rank r's map says travels to q is what q's receive plan (dory_partition_recv_plan) expects"""
    d = os.path.join(ROOT, "tests", "golden", case)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    assert bins, case
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    pobjs = [da.Partition.load(b) for b in bins]
    views = [p.view() for p in pobjs]
    for direction, key in ((0, "fwdLists"), (1, "bwdLists")):
        for r, (p, v) in enumerate(zip(pobjs, views)):
            N = int(v["localVtxCnt"])
            row_ptr, row_slots = check(da, N, v[key])
            assert np.diff(row_ptr.astype(np.int64)).max(initial=0) <= len(pobjs) - 1       # once per peer that needs the row
            recv = p.recv_plan(parts, direction)
            for q in range(len(pobjs)):
                assert len(recv[q]) == len(views[q][key][r]), (case, direction, r, q)
