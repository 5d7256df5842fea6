"""Option halo_exact_rows without a GPU: the numpy statement of the exact layout (tests/halo_exact_ref.py) against itself and the
padded form, and what the case list of tests/test_gpu_halo_exact_rows.py reaches -- every way the stream of n x cols floats can
end, quads that straddle rows, both kernel pairs, empty and one-row lists, more rows than one workgroup takes, repeated rows."""
import numpy as np

import halo_exact_ref as hx


def test_pack_is_one_dense_stream_and_unpack_writes_whole_rows():
    rng = np.random.default_rng(0)
    for cols in hx.COLS:
        ld = hx.pad_ld(cols)
        x = np.zeros((hx.N_LOCAL, ld), np.float32)
        x[:, :cols] = rng.standard_normal((hx.N_LOCAL, cols)).astype(np.float32)
        rows = hx.send_list(7, cols)
        buf = hx.pack(x, rows, cols)
        assert buf.shape == (7 * cols,)
        for i, r in enumerate(rows):
            assert np.array_equal(buf[i * cols:(i + 1) * cols], x[r, :cols])
        # the padded form carries the same values plus the owner's zeros
        pb = hx.pack_padded(x, rows, cols).reshape(7, ld)
        assert np.array_equal(pb[:, :cols].reshape(-1), buf) and not pb[:, cols:].any()
        # unpack into poisoned ghost rows: the same raw bits as copying the padded rows whole
        slots = hx.recv_slots(7, cols)
        ghost = np.full((7, ld), np.nan, np.float32)
        hx.unpack(ghost, slots, buf, cols)
        want = np.empty((7, ld), np.float32)
        want[slots] = pb
        assert np.array_equal(ghost.view(np.uint32), want.view(np.uint32))


def test_peer_offsets_are_rows_times_cols():
    counts = [0, 5, 0, 7, 1]
    c, o = hx.peer_offsets(counts, 41)
    assert list(c) == [0, 205, 0, 287, 41] and list(o) == [0, 0, 205, 205, 492]
    c0, o0 = hx.peer_offsets(counts, hx.pad_ld(41))
    assert list(c0) == [0, 320, 0, 448, 64] and list(o0) == [0, 0, 320, 320, 768]


def test_case_list_reaches_every_path():
    assert set(c for c, _ in hx.CASES) == set(hx.COLS) and set(hx.RECV_ROWS) == set(hx.COLS)
    exact = [c for c in hx.COLS if hx.takes_exact_kernels(c)]
    # every residue of n x cols mod 4, for the pack (all of ROWS per width) and for the unpack, on the new kernels
    assert {(n * c) % 4 for c in exact for n in hx.ROWS if n} == {0, 1, 2, 3}
    assert {(n * c) % 4 for c, n in hx.CASES if hx.takes_exact_kernels(c) and n} == {0, 1, 2, 3}
    for c in (3, 5, 25, 41):            # and per odd width, both sides: all four
        assert {(n * c) % 4 for n in hx.ROWS if n} == {0, 1, 2, 3}
        assert {(n * c) % 4 for n in hx.RECV_ROWS[c] if n} == {0, 1, 2, 3}, c
    # a quad that straddles three rows and more (cols = 1: four rows), one that straddles two or three (cols = 3), two (the rest)
    assert 1 in exact and 3 in exact
    # the existing kernels with an exact width below the padding, the untouched path, and rows beyond one 128-float slab
    assert any(c % 4 == 0 and c < hx.pad_ld(c) for c in hx.COLS)
    assert any(c == hx.pad_ld(c) and c > 1 for c in hx.COLS)
    assert any(c > 128 and hx.takes_exact_kernels(c) for c in hx.COLS)
    # empty and one-row lists on both sides
    assert {0, 1} <= set(hx.ROWS)
    assert {0, 1} <= {n for c, n in hx.CASES if hx.takes_exact_kernels(c)}
    # more rows than one workgroup's share, both sides, on the narrowest and on a typical width; the share keeps 16-byte starts
    for c in exact:
        assert hx.rows_per_workgroup(c) % 4 == 0 and hx.rows_per_workgroup(c) * c >= 4096
    for c in (1, 41, 602):
        assert max(hx.ROWS) > hx.rows_per_workgroup(c)
        assert max(hx.RECV_ROWS[c]) > hx.rows_per_workgroup(c), c
    # send lists repeat rows; receive lists are permutations
    for n in hx.ROWS:
        rows = hx.send_list(n, 1)
        assert rows.size == n and (n < 2 or np.unique(rows).size < n) and (n == 0 or rows.max() < hx.N_LOCAL)
        assert sorted(hx.recv_slots(n, 1)) == list(range(n))
    # values stay exact integers in fp32
    assert hx.wire_values(max(hx.ROWS), max(hx.COLS)).max() < 2 ** 24
    assert np.unique(hx.local_values(602)).size == hx.N_LOCAL * 602


def test_case_graphs_have_the_ghost_counts():
    import aggregate_ref as ar
    for n in (0, 3, 257):
        g = ar.graph(hx.graph_name(n))
        assert g["localVtxCnt"] == hx.N_LOCAL and g["srcGhostCnt"] == n and g["dstGhostCnt"] == n
        assert (np.asarray(g["rowIdx"]) < hx.N_LOCAL + n).all() and (np.asarray(g["colIdx"]) < hx.N_LOCAL + n).all()
