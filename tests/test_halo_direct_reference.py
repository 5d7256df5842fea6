"""dory_partition_wire_order (option halo_direct_recv's host half, no GPU needed) against the numpy mirror of
tests/halo_direct_ref.py, on every golden partition and both directions: the order is a permutation and is the list
dory_partition_recv_plan emits, the renumbered ids map back to the original array exactly, pointers and values are not
touched, the partition object is left as it was (view and saved bytes), contiguous parts give the identity, an empty rank and
a rank without ghosts work, and the hash-partitioned golden really has a non-identity order."""
import os

import numpy as np
import pytest

import halo_direct_ref as hd


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    if not os.path.exists(dorylus_amd.LIB_PATH):
        pytest.skip("library not built (run __graft_entry__.build())")
    return dorylus_amd


def _snapshot(view):
    return {k: (np.array(v, copy=True) if isinstance(v, np.ndarray) else [np.array(x, copy=True) for x in v] if isinstance(v, list) else v)
            for k, v in view.items()}


def _same_view(a, b):
    assert set(a) == set(b)
    for k in a:
        if isinstance(a[k], list):
            assert len(a[k]) == len(b[k]) and all(np.array_equal(x, y) for x, y in zip(a[k], b[k])), k
        else:
            assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("direction", [0, 1])
@pytest.mark.parametrize("name", hd.GOLDEN)
def test_wire_order_matches_the_mirror_and_the_recv_plan(da, name, direction, tmp_path):
    pobjs, parts = hd.golden(da, name)
    gk, ik, pk, vk = hd.SIDES[direction]
    for r, part in enumerate(pobjs):
        before = _snapshot(part.view())
        part.save(str(tmp_path / "before.bin"))
        order, idxs = part.wire_order(parts, direction)
        v = part.view()
        N, P, G = int(v["localVtxCnt"]), int(v["numNodes"]), len(v[gk])
        # a permutation of the ghost slots, the concatenated lists of dory_partition_recv_plan, the mirror's
        assert order.dtype == np.uint32 and sorted(order.tolist()) == list(range(G)), (name, r)
        plan = part.recv_plan(parts, direction)
        assert np.array_equal(order, np.concatenate(plan + [np.zeros(0, np.uint32)])), (name, r, "recv_plan")
        want, counts = hd.wire_order(v[gk], parts, P)
        assert np.array_equal(order, want) and counts == [len(x) for x in plan], (name, r, "mirror")
        # the renumbered copy: the mirror's, same length and local ids, maps back to the original exactly
        assert np.array_equal(idxs, hd.renumber(v[ik], N, order)), (name, r, "renumbered ids")
        assert idxs.shape == v[ik].shape and np.array_equal(idxs < N, v[ik] < N) and np.array_equal(idxs[idxs < N], v[ik][v[ik] < N])
        assert (idxs < N + G).all()
        assert np.array_equal(hd.caller_ids(idxs, N, order), v[ik]), (name, r, "maps back")
        # a ghost's r-th position is the peer segment it arrives in
        off = np.concatenate([[0], np.cumsum(counts)])
        for q in range(P):
            assert (parts[v[gk][order[off[q]:off[q + 1]]]] == q).all(), (name, r, q)
        # nothing of the partition moved: its view (pointers and values included) and the bytes it saves
        _same_view(before, part.view())
        part.save(str(tmp_path / "after.bin"))
        assert (tmp_path / "before.bin").read_bytes() == (tmp_path / "after.bin").read_bytes(), (name, r)


def test_hash_partition_has_a_wire_order_that_is_not_the_identity(da):
    """parts_toy60_p4_hash interleaves the owners: without this the feature could pass with nothing renumbered"""
    pobjs, parts = hd.golden(da, "parts_toy60_p4_hash")
    moved = 0
    for part in pobjs:
        for direction in (0, 1):
            order, idxs = part.wire_order(parts, direction)
            v = part.view()
            assert len(order) > 0
            assert not np.array_equal(order, np.arange(len(order))), "order == arange on the hash partition"
            moved += int((idxs != v[hd.SIDES[direction][1]]).sum())
    assert moved > 0


def test_contiguous_parts_give_the_identity(da):
    """ghost slots ascend with global id; where the owners do too (parts non-decreasing in vertex id) the rows arrive in slot order"""
    rng = np.random.default_rng(3)
    V, E, P = 90, 700, 4
    src, dst = rng.integers(0, V, E).astype(np.uint32), rng.integers(0, V, E).astype(np.uint32)
    parts = (np.arange(V) * P // V).astype(np.int32)
    assert (np.diff(parts) >= 0).all()
    for r in range(P):
        part = da.Partition.build(src, dst, parts, r, P)
        v = part.view()
        for direction in (0, 1):
            order, idxs = part.wire_order(parts, direction)
            assert len(order) > 0 and np.array_equal(order, np.arange(len(order))), (r, direction)
            assert np.array_equal(idxs, v[hd.SIDES[direction][1]]), (r, direction)


def test_empty_rank_and_rank_without_ghosts(da):
    pobjs, parts = hd.golden(da, "parts_toy40_p3_empty")
    empty = [p for p in pobjs if int(p.view()["localVtxCnt"]) == 0]
    assert empty, "the golden has an empty rank"
    for part in empty:
        for direction in (0, 1):
            order, idxs = part.wire_order(parts, direction)
            assert order.size == 0 and idxs.size == 0
    # two components, one per rank: edges, but no ghosts
    src = np.array([0, 1, 2, 5, 6, 7, 1], np.uint32)
    dst = np.array([1, 2, 0, 6, 7, 5, 0], np.uint32)
    parts = np.array([0, 0, 0, 0, 1, 1, 1, 1], np.int32)
    for r in range(2):
        part = da.Partition.build(src, dst, parts, r, 2)
        v = part.view()
        assert int(v["srcGhostCnt"]) == 0 and int(v["dstGhostCnt"]) == 0
        for direction in (0, 1):
            order, idxs = part.wire_order(parts, direction)
            assert order.size == 0 and np.array_equal(idxs, v[hd.SIDES[direction][1]]) and idxs.size > 0
    # a single partition
    one = da.Partition.build(src, dst, np.zeros(8, np.int32), 0, 1)
    order, idxs = one.wire_order(np.zeros(8, np.int32), 0)
    assert order.size == 0 and np.array_equal(idxs, one.view()["rowIdx"])


def test_bad_arguments_are_refused(da):
    pobjs, parts = hd.golden(da, "parts_toy60_p2")
    with pytest.raises(da.DoryError):
        pobjs[0].wire_order(parts, 2)
    bad = parts.copy()
    bad[pobjs[0].view()["srcGhost"][0]] = 9          # an owner that is no rank
    with pytest.raises(da.DoryError):
        pobjs[0].wire_order(bad, 0)
