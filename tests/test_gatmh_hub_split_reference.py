"""dory_gatmh_row_gather_hub_split without a GPU: the chunk plan of an adjacency (dory_row_chunk_plan, include/dorylus_host.h -- the plan
the context builds for the row-gather kernels), the chunk-and-merge arithmetic restated in numpy (tests/gatmh_hub_split_ref.py) against
the float64 oracle, the entry points and what they refuse without a context."""
import ctypes
import glob
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNKS = (64, 512)


def _check_plan(ptr, chunk):
    """every entry of every row covered exactly once, in order; exactly the rows over `chunk` are cut, into ceil(deg / chunk) chunks"""
    import dorylus_amd as da
    ptr = np.asarray(ptr, np.uint64)
    rows, first, crow, e0, e1 = da.row_chunk_plan(ptr, chunk)
    deg = np.diff(ptr.astype(np.int64))
    want_rows = np.nonzero(deg > chunk)[0]
    assert np.array_equal(rows, want_rows), (rows, want_rows)
    assert first[0] == 0 and first[-1] == crow.size and np.all(np.diff(first.astype(np.int64)) >= 2)
    for i, v in enumerate(rows):
        c0, c1 = int(first[i]), int(first[i + 1])
        assert c1 - c0 == -(-int(deg[v]) // chunk), (v, deg[v], c1 - c0)
        assert np.all(crow[c0:c1] == v)
        assert e0[c0] == ptr[v] and e1[c1 - 1] == ptr[v + 1]
        assert np.array_equal(e0[c0 + 1:c1], e1[c0:c1 - 1])                 # consecutive: nothing skipped, nothing twice
        assert np.all(e1[c0:c1 - 1] - e0[c0:c1 - 1] == chunk)               # full chunks, then the shorter (never empty) last one
        assert 0 < e1[c1 - 1] - e0[c1 - 1] <= chunk
    return rows, first


@pytest.mark.parametrize("chunk", CHUNKS)
def test_plan_of_the_golden_partition(chunk):
    import partition_oracle as po
    dd = os.path.join(ROOT, "tests", "golden", "parts_hub3000_p2")
    bins = sorted(glob.glob(os.path.join(dd, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    assert len(bins) == 2
    cut = 0
    for b in bins:
        g = po.parse_graph_bin(open(b, "rb").read())
        for key in ("colPtr", "rowPtr"):
            rows, first = _check_plan(g[key], chunk)
            cut += len(rows)
    assert cut >= 1          # (the row of 3 000 entries)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_plan_of_a_random_graph_with_a_200_edge_hub_and_the_edges_of_the_rule(chunk):
    rng = np.random.default_rng(chunk)
    deg = rng.integers(0, 12, 300)
    deg[7] = 200
    deg[20:23] = (chunk - 1, chunk, chunk + 1)
    deg[40] = 3 * chunk
    ptr = np.concatenate([[0], np.cumsum(deg)]).astype(np.uint64)
    rows, first = _check_plan(ptr, chunk)
    nch = dict(zip(rows.tolist(), np.diff(first.astype(np.int64)).tolist()))
    assert 20 not in nch and 21 not in nch            # chunk - 1 and exactly chunk entries: not cut
    assert nch[22] == 2 and nch[40] == 3              # chunk + 1: two chunks (chunk, 1); 3 chunk: three full ones
    assert (7 in nch) == (200 > chunk) and nch.get(7, 4) == 4


def test_plan_of_rows_that_are_never_cut_and_refusals():
    import dorylus_amd as da
    rows, first, crow, e0, e1 = da.row_chunk_plan(np.array([0, 5, 5, 69], np.uint64), 64)
    assert rows.size == 0 and crow.size == 0 and first.tolist() == [0]
    lib = da.load()
    ptr = np.array([0, 5, 3], np.uint64)
    n = ctypes.c_uint32()
    assert lib.dory_row_chunk_plan(ptr.ctypes.data_as(ctypes.c_void_p), 2, 64, ctypes.byref(n), None, None, None, None, None, None) != 0
    assert lib.dory_row_chunk_plan(None, 2, 64, ctypes.byref(n), None, None, None, None, None, None) != 0
    ptr = np.array([0, 5, 300], np.uint64)
    assert lib.dory_row_chunk_plan(ptr.ctypes.data_as(ctypes.c_void_p), 2, 0, ctypes.byref(n), None, None, None, None, None, None) != 0


def test_entry_points_exist_and_refuse_a_null_context():
    import dorylus_amd as da
    assert "dory_gatmh_row_gather_hub_split" in da.SYMBOLS and "dory_gatmh_row_gather_hub_split_stats" in da.SYMBOLS
    lib = da.load()
    assert lib.dory_gatmh_row_gather_hub_split(None, 64) != 0
    assert lib.dory_gatmh_row_gather_hub_split_stats(None, *[None] * 7) != 0
    assert callable(da.Context.gatmh_row_gather_hub_split) and callable(da.Context.gatmh_row_gather_hub_split_stats)


@pytest.mark.parametrize("K,D", [(4, 16), (32, 2), (1, 25)])
def test_chunk_and_merge_arithmetic_against_the_oracle(K, D):
    """one layer on the 240-vertex hub graph (a 200-in-edge destination, a 200-out-edge source) at chunk sizes 64 (four chunks, the self
    edge in a last chunk of nine entries) and 0 (one pass), in float32, against oracle/gat_mh_oracle.py at 1e-4"""
    import gat_mh_oracle as go
    import partition_oracle as po
    import gatmh_hub_split_ref as ref
    from helpers import rel_err
    V, E = 240, 2600
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    g = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    assert np.diff(g["colPtr"].astype(np.int64)).max() >= 200 and np.diff(g["rowPtr"].astype(np.int64)).max() >= 200
    H = rng.uniform(-1, 1, (V, 24))
    W = rng.standard_normal((24, K * D)) / np.sqrt(24)
    a_l, a_r = rng.standard_normal(K * D) * 0.3, rng.standard_normal(K * D) * 0.3
    dO = rng.standard_normal((V, K * D))
    fw = go.layer_forward(g, H, W, a_l, a_r, K)
    bw = go.layer_backward(g, H, W, a_l, a_r, fw, dO)
    colptr, rowidx = g["colPtr"].astype(np.int64), g["rowIdx"].astype(np.int64)
    rowptr, colidx = g["rowPtr"].astype(np.int64), g["colIdx"].astype(np.int64)
    m_by_chunk = {}
    for chunk in (64, 0):
        o, op, m, den, dpos = ref.forward(colptr, rowidx, fw["Z"], fw["el"], fw["er"], K, chunk)
        assert o.dtype == np.float32 and np.isfinite(o).all()
        assert rel_err(o, fw["O"]) < 1e-4, (chunk, rel_err(o, fw["O"]))
        assert np.abs(m - fw["m"]).max() < 1e-4 * max(1.0, np.abs(fw["m"]).max()), chunk
        m_by_chunk[chunk] = m
        assert rel_err(den, fw["den"]) < 1e-4, chunk
        # op / dpos: the positive-branch part of o and of the attention mass
        pos = (fw["el"][fw["src"]] + fw["er"][fw["dst"]]) > 0
        want = np.zeros((V, K, D))
        np.add.at(want, fw["dst"], (fw["alpha"] * pos)[:, :, None] * fw["Z"].reshape(V, K, D)[fw["src"]])
        assert rel_err(op, want.reshape(V, K * D)) < 1e-4, chunk
        wantp = np.zeros((V, K))
        np.add.at(wantp, fw["dst"], fw["alpha"] * pos)
        assert np.abs(dpos - wantp).max() < 1e-4, chunk
        t, der = ref.dst_side(colptr, rowidx, fw["Z"], fw["el"], fw["er"], m, den, dO, K, chunk)
        assert rel_err(t, bw["t"]) < 1e-4 and rel_err(der, bw["d_er"]) < 1e-4, (chunk, rel_err(t, bw["t"]), rel_err(der, bw["d_er"]))
        dl, dz = ref.src_side(rowptr, colidx, fw["Z"], fw["el"], fw["er"], m, den, t, der, dO, a_l, a_r, K, chunk)
        assert rel_err(dl, bw["d_el"]) < 1e-4 and rel_err(dz, bw["dZ"]) < 1e-4, (chunk, rel_err(dl, bw["d_el"]), rel_err(dz, bw["dZ"]))
    assert np.array_equal(m_by_chunk[64], m_by_chunk[0])          # the maximum of the chunk maxima IS the row's maximum: exact
    # the cut rows are the hub destination / the hub source, and nothing else
    assert [len(ref.row_chunks(colptr, v, 64)) for v in (6, 7)] == [1, 4]
    assert ref.row_chunks(colptr, 7, 64)[-1][2] and not ref.row_chunks(colptr, 7, 64)[0][2]
