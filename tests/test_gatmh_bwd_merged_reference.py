"""tests/gatmh_bwd_merged_ref.py, the numpy statement of the merged rows of dory_gatmh_bwd_merged_exchange, against the two
separate exchanges it replaces (no GPU): on the golden partitions, with the plans of tests/halo_plan_ref.py and random do / st,
unpack(route(pack)) leaves in every rank's bg_do / bg_st exactly the rows the owners hold, bit for bit what routing the two padded
tensors one after the other leaves, padding included; and the width of the do part follows the rule of the header."""
import glob
import os

import numpy as np
import pytest

import gatmh_bwd_merged_ref as mr
from halo_plan_ref import halo_plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("parts_toy60_p2", "parts_toy60_p4_hash")
SHAPES = ((41, 1), (44, 1), (128, 8))          # (cols of do, heads)


def _views(name):
    import dorylus_amd as da
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    objs = [da.Partition.load(b) for b in bins]
    return objs, [o.view() for o in objs], parts


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("cols,exact,w", [(41, 0, 64), (41, 1, 44), (44, 0, 64), (44, 1, 44), (128, 0, 128), (128, 1, 128)])
def test_width_of_the_do_part(cols, exact, w):
    assert mr.wire_w(cols, exact) == w and w % 4 == 0 and w <= mr.pad_ld(cols)
    for K in (1, 2, 8):
        R, ww, s = mr.wire_row(cols, K, exact)
        assert (R, ww, s) == (w + 4 * K, w, 4 * K) and R % 4 == 0


def test_bytes_per_row_of_the_reddit_shape():
    """602-128-41 with heads 8 / 1 (the issue's arithmetic): hidden 512 + 128 -> 640 B; last 256 + 128 = 384 -> 272 B, 192 B exact"""
    assert 4 * mr.pad_ld(128) + 4 * mr.pad_ld(32) == 640 == 4 * mr.wire_row(128, 8, 0)[0] == 4 * mr.wire_row(128, 8, 1)[0]
    assert 4 * mr.pad_ld(41) + 4 * mr.pad_ld(4) == 384
    assert 4 * mr.wire_row(41, 1, 0)[0] == 272 and 4 * mr.wire_row(41, 1, 1)[0] == 192


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("cols,K", SHAPES)
@pytest.mark.parametrize("exact", [0, 1])
def test_merged_rows_leave_what_two_exchanges_leave(case, cols, K, exact):
    objs, views, parts = _views(case)
    P = len(views)
    plans = [halo_plan(views[r], parts, r, P)[1] for r in range(P)]             # the backward plans: (send lists, recv lists)
    send = [[np.asarray(x, np.int64) for x in plans[r][0]] for r in range(P)]
    recv = [[np.asarray(x, np.int64) for x in plans[r][1]] for r in range(P)]
    assert sum(len(x) for r in range(P) for x in send[r]) > 0
    rng = np.random.default_rng([3, cols, K, exact, P])
    ld, ld_st = mr.pad_ld(cols), mr.pad_ld(4 * K)
    R, w, _ = mr.wire_row(cols, K, exact)
    do, st = [], []
    for r in range(P):
        N = int(views[r]["localVtxCnt"])
        do.append(rng.standard_normal((N, cols)).astype(np.float32))
        s = np.zeros((N, ld_st), np.float32)
        s[:, :4 * K] = rng.standard_normal((N, 4 * K))
        st.append(s)
    G = [int(views[r]["dstGhostCnt"]) for r in range(P)]
    # merged: one pack, one route, one unpack per rank
    bufs = [mr.pack(do[r], st[r], K, w, send[r]) for r in range(P)]
    for r in range(P):
        assert bufs[r].dtype == np.float32 and bufs[r].size == sum(len(x) for x in send[r]) * R
    got = mr.route(bufs, R, send, recv)
    merged = [mr.unpack(got[p], K, w, recv[p], G[p], ld, ld_st) for p in range(P)]
    # the two tensors one after the other, at their padded widths (what exchange_rows ships today)
    pad = lambda t, wd: np.concatenate([t, np.zeros((t.shape[0], wd - t.shape[1]), np.float32)], axis=1)
    for p in range(P):
        bg_do, bg_st = np.full((G[p], ld), np.nan, np.float32), np.full((G[p], ld_st), np.nan, np.float32)
        for r in range(P):
            if len(send[r][p]):
                bg_do[recv[p][r]] = pad(do[r], ld)[send[r][p]]
                bg_st[recv[p][r]] = st[r][send[r][p]]
        assert not np.isnan(bg_do).any() and not np.isnan(bg_st).any(), (p, "the plans cover every ghost slot")
        assert np.array_equal(_bits(merged[p][0]), _bits(bg_do)), (case, p, "bg_do")
        assert np.array_equal(_bits(merged[p][1]), _bits(bg_st)), (case, p, "bg_st")
        # exactly the rows the owners hold: ghost slot k of rank p is global vertex dstGhost[k]
        gv = np.asarray(views[p]["dstGhost"], np.int64)
        for k in range(G[p]):
            o = int(parts[gv[k]])
            lv = int(np.searchsorted(np.asarray(views[o]["localToGlobal"], np.int64), gv[k]))
            assert int(views[o]["localToGlobal"][lv]) == gv[k]
            assert np.array_equal(_bits(merged[p][0][k, :cols]), _bits(do[o][lv])) and not merged[p][0][k, cols:].any(), (case, p, k)
            assert np.array_equal(_bits(merged[p][1][k]), _bits(st[o][lv])), (case, p, k)
    for o in objs:
        o.close()
