"""tests/gatmh_halo_bf16_ref.py, the numpy statement of the merged row [do as bf16 | st as fp32] of dory_gatmh_halo_bf16, against
packing hb.rounded(do) and st separately with tests/gatmh_bwd_merged_ref.py (no GPU): the do part of every row holds the bf16 bits of
the rounded fp32 merged row's do part (and zeros behind cols), the st part its st part bit for bit; unpack(route(pack)) leaves in
every rank's bg_do / bg_st what routing the rounded do and st leaves; widths 16, 32, 41 (exact: 48 elements, where the fp32 merged row
has 44), 64, 128 and 256, K in 1, 2, 4, 8, send lists that repeat a row and a peer with an empty list."""
import numpy as np
import pytest

import gatmh_bwd_merged_ref as mr
import gatmh_halo_bf16_ref as gr
import halo_bf16_ref as hb

WIDTHS = (16, 32, 41, 64, 128, 256)
HEADS = (1, 2, 4, 8)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("cols,exact,w", [(16, 0, 32), (16, 1, 16), (41, 0, 64), (41, 1, 48), (44, 1, 48), (48, 1, 48), (64, 1, 64), (128, 0, 128),
                                          (250, 1, 256), (256, 1, 256)])
def test_width_of_the_do_part(cols, exact, w):
    assert gr.wire_w(cols, exact) == w and w % 8 == 0 and w <= gr.pad_ld(cols)
    for K in HEADS:
        R, dof, s, ww = gr.wire_row(cols, K, exact)
        assert (R, dof, s, ww) == (w // 2 + 4 * K, w // 2, 4 * K, w) and R % 4 == 0 and (2 * w) % 16 == 0
    assert mr.wire_w(41, 1) == 44 and gr.wire_w(41, 1) == 48          # (a multiple of 8 elements, not of 4 floats)


def test_bytes_per_row_of_the_reddit_shape():
    """602-128-41 with heads 8 / 1 (the issue's arithmetic): merged hidden 640 -> 384 B, last 272 -> 144 B (112 B exact); forward z
    512 -> 256 B and 256 -> 128 B (88 B exact)"""
    assert 4 * mr.wire_row(128, 8, 0)[0] == 640 and 4 * gr.wire_row(128, 8, 0)[0] == 384 == 4 * gr.wire_row(128, 8, 1)[0]
    assert 4 * mr.wire_row(41, 1, 0)[0] == 272 and 4 * gr.wire_row(41, 1, 0)[0] == 144 and 4 * gr.wire_row(41, 1, 1)[0] == 112
    assert 2 * hb.row_elems(128, 0) == 256 and 2 * hb.row_elems(41, 0) == 128 and 2 * hb.row_elems(41, 1) == 88


def _lists(N, P, rng):
    """per-peer send lists: a row listed for every peer, rows listed for none, a list with a row twice, an empty peer"""
    lists = [list(rng.choice(N, size=min(N, 5 + p), replace=False)) for p in range(P)]
    for l in lists:
        l.append(3)                                         # row 3 travels to every peer
    lists[1].append(lists[1][0])                            # ... and one row twice to the same peer
    lists[0] = []                                           # (the sender itself)
    lists[P - 1] = []                                       # an empty peer
    return [[int(x) for x in l] for l in lists]


@pytest.mark.parametrize("cols", WIDTHS)
@pytest.mark.parametrize("K", HEADS)
@pytest.mark.parametrize("exact", [0, 1])
def test_rows_against_the_rounded_fp32_merged_rows(cols, K, exact):
    rng = np.random.default_rng([5, cols, K, exact])
    N, P = 23, 4
    do = hb.patterns(N * cols, seed=cols + K, finite=True).reshape(N, cols).copy()        # ties, denormals, signed zeros among them
    st = np.zeros((N, mr.pad_ld(4 * K)), np.float32)
    st[:, :4 * K] = hb.patterns(N * 4 * K, seed=7 * K + cols).reshape(N, 4 * K)
    lists = _lists(N, P, rng)
    T = sum(len(l) for l in lists)
    R, dof, k4, w = gr.wire_row(cols, K, exact)
    buf = gr.pack(do, st, K, w, lists)
    assert buf.dtype == np.float32 and buf.size == T * R
    # the same rows packed separately as fp32 merged rows of the rounded do, at the bf16 form's width
    ref = mr.pack(hb.rounded(do), st, K, w, lists).reshape(T, w + 4 * K)
    rows = buf.view(np.uint8).reshape(T, 4 * R)
    got_do = np.ascontiguousarray(rows[:, :2 * w]).view(np.uint16)
    assert np.array_equal(got_do, (_bits(ref[:, :w]) >> 16).astype(np.uint16)) and not (_bits(ref[:, :w]) & 0xFFFF).any()
    assert not got_do[:, cols:].any(), "zeros behind cols"
    assert np.array_equal(np.ascontiguousarray(rows[:, 2 * w:]).view(np.uint32), _bits(ref[:, w:])), "st keeps its bits"
    # one rank's rows through an all-to-all-v into three receivers, then the unpack: whole rows of both tensors
    ld, ld_st = mr.pad_ld(cols), mr.pad_ld(4 * K)
    send = [lists] + [[[] for _ in range(P)] for _ in range(P - 1)]
    recv = [[[] for _ in range(P)] for _ in range(P)]
    for p in range(1, P):
        recv[p][0] = list(rng.permutation(len(lists[p])))
    routed = gr.route([buf] + [np.zeros(0, np.float32)] * (P - 1), R, send, recv)
    routed_ref = mr.route([ref.reshape(-1)] + [np.zeros(0, np.float32)] * (P - 1), w + 4 * K, send, recv)
    for p in range(1, P):
        G = len(lists[p])
        poison = np.full((G, ld), 7.0, np.float32), np.full((G, ld_st), 7.0, np.float32)
        a = gr.unpack(routed[p], K, w, recv[p], G, ld, ld_st, *poison)
        b = mr.unpack(routed_ref[p], K, w, recv[p], G, ld, ld_st, *poison)
        assert np.array_equal(_bits(a[0]), _bits(b[0])) and np.array_equal(_bits(a[1]), _bits(b[1])), (p, "ghost rows")
        if G:
            assert not a[0][:, w:].any() and not a[1][:, 4 * K:].any()
            assert np.array_equal(_bits(a[0][recv[p][0], :cols]), _bits(hb.rounded(do[lists[p]])))
