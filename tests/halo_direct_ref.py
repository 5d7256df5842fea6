"""Option halo_direct_recv in plain numpy: the wire order of a partition's ghosts and the renumbered index arrays
(dory_partition_wire_order, dorylus_amd/host/partition.cpp).

A halo exchange delivers rows peer by peer (rank order), each peer's rows in the order of its send list: its local ids
ascending, i.e. ascending global id.  order[r] is the ghost slot k (local id N + k) of the r-th row that arrives.  With the
option a context stores ghost row r at row r, so the adjacency it is given names that ghost N + r: every id N + k of the
index array becomes N + inv[k], inv the inverse of order.  tests/test_halo_direct_reference.py compares the library with this
where there is no GPU; tests/test_gpu_halo_direct_recv.py uses it to build what a direct dory_graph_upload caller hands over."""
import glob
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = ("parts_toy60_p2", "parts_toy40_p3_empty", "parts_toy60_p4_hash", "parts_toy97_p8_und")
SIDES = {0: ("srcGhost", "rowIdx", "colPtr", "cscVal"), 1: ("dstGhost", "colIdx", "rowPtr", "csrVal")}   # ghosts, index, pointer, value arrays of a direction


def golden(da, name):
    """(da.Partition per rank, parts vector) of tests/golden/<name>: graph.<id>.bin as the reference's loader wrote them"""
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


def wire_order(ghost_gvids, parts, P):
    """order[r] = ghost slot of the r-th received row: the slots owned by rank 0 (ascending), then rank 1's, ..."""
    owners = np.asarray(parts)[np.asarray(ghost_gvids, np.int64)]
    per = [np.nonzero(owners == q)[0] for q in range(P)]
    return np.concatenate(per + [np.zeros(0, np.int64)]).astype(np.uint32), [len(x) for x in per]


def inverse(order):
    inv = np.empty(len(order), np.uint32)
    inv[np.asarray(order, np.int64)] = np.arange(len(order), dtype=np.uint32)
    return inv


def renumber(idx, N, order):
    """the index array with ghost id N + k replaced by N + inv[k]; local ids and the edge order stay"""
    idx = np.asarray(idx, np.uint32)
    out = idx.copy()
    m = idx >= N
    out[m] = N + inverse(order)[idx[m] - N]
    return out


def caller_ids(idx_wire, N, order):
    """back: ghost id N + r of a renumbered array names the caller's ghost N + order[r]"""
    idx_wire = np.asarray(idx_wire, np.uint32)
    out = idx_wire.copy()
    m = idx_wire >= N
    out[m] = N + np.asarray(order, np.uint32)[idx_wire[m] - N]
    return out


def wired_graph(g, orders):
    """a graph_upload dict with both index arrays renumbered: what a caller of dory_graph_upload promises under the option"""
    h = dict(g)
    N = int(g["localVtxCnt"])
    h["rowIdx"] = renumber(g["rowIdx"], N, orders[0])
    h["colIdx"] = renumber(g["colIdx"], N, orders[1])
    return h
