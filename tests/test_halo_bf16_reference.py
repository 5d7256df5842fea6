"""tests/halo_bf16_ref.py against torch on the CPU (no GPU): the rounding on the bits is torch.Tensor.to(torch.bfloat16) on random
bit patterns without NaN and on the named cases (ties to even in both directions and their neighbours, denormals, +-0, +-FLT_MAX ->
inf, +-inf); the packed layouts (padded and exact, trailing zeros, bytes per row of the header's table); the unpack that writes whole
ghost rows; pack -> unpack is the rounding; rounding is idempotent; the rule; the per-peer float offsets of the host transport."""
import numpy as np
import pytest

import halo_bf16_ref as hb
import halo_exact_ref as hx


def _torch_bits(x):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(x, np.float32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy().view(np.uint16)


def test_rounding_is_torchs_on_random_patterns_and_named_cases():
    x = np.concatenate([hb.patterns(199264 - hb.named_patterns().size, seed=3), hb.named_patterns().view(np.float32)])
    assert x.size == 199264 and not np.isnan(x).any()
    assert np.array_equal(hb.round_bits(x), _torch_bits(x))


def test_named_cases():
    r = lambda u: int(hb.round_bits(np.array([u], np.uint32).view(np.float32))[0])
    assert r(0x3F808000) == 0x3F80 and r(0x3F818000) == 0x3F82               # ties: down to even, up to even
    assert r(0x3F807FFF) == 0x3F80 and r(0x3F808001) == 0x3F81               # one ulp either side of the first tie
    assert r(0x3F817FFF) == 0x3F81 and r(0x3F818001) == 0x3F82
    assert r(0x00000001) == 0 and r(0x00008000) == 0 and r(0x00008001) == 1 and r(0x00018000) == 2      # denormals, ties among them
    assert r(0x007FFFFF) == 0x0080                                            # the largest denormal rounds into the smallest normal
    assert r(0x00000000) == 0x0000 and r(0x80000000) == 0x8000                # +-0 keep their sign
    assert r(0x7F7FFFFF) == 0x7F80 and r(0xFF7FFFFF) == 0xFF80                # +-FLT_MAX -> +-inf
    assert r(0x7F800000) == 0x7F80 and r(0xFF800000) == 0xFF80
    for u in hb.named_patterns():
        assert r(int(u)) == int(_torch_bits(np.array([u], np.uint32).view(np.float32))[0]), hex(int(u))


def test_generator_has_no_nan_and_holds_the_named_cases():
    for finite in (False, True):
        x = hb.patterns(5000, seed=1, finite=finite)
        assert not np.isnan(x).any()
        assert not finite or np.isfinite(x).all()
    u = hb.patterns(5000, seed=1).view(np.uint32)
    for v in hb.NAMED.values():
        assert v in u, hex(v)
    lv = hb.local_values(hx.N_LOCAL, 41)
    assert lv.shape == (hx.N_LOCAL, 41) and not np.isnan(lv).any()
    assert (lv.view(np.uint32) == 0x3F808000).any() and np.isinf(lv).any()


def test_rounding_is_idempotent_and_widening_exact():
    x = hb.patterns(50000, seed=5)
    once = hb.rounded(x)
    assert np.array_equal(hb.rounded(once).view(np.uint32), once.view(np.uint32))
    assert np.array_equal(hb.round_bits(once), hb.round_bits(x))
    assert (once.view(np.uint32) & 0xFFFF == 0).all()


@pytest.mark.parametrize("cols", hx.COLS)
def test_row_elems_and_bytes(cols):
    ld = hx.pad_ld(cols)
    p, e = hb.row_elems(cols, False), hb.row_elems(cols, True)
    assert p % 4 == 0 and e % 4 == 0 and cols <= e < cols + 4 and e <= p
    assert p == (ld if ld > 1 else 4)
    assert 2 * p <= max(4 * ld, 8) and (2 * e) % 8 == 0


def test_bytes_per_row_of_the_headers_table():
    for cols, want in ((128, (512, 512, 256, 256)), (64, (256, 256, 128, 128)), (48, (256, 192, 128, 96)), (41, (256, 164, 128, 88))):
        got = (4 * hx.pad_ld(cols), 4 * cols, 2 * hb.row_elems(cols, False), 2 * hb.row_elems(cols, True))
        assert got == want, (cols, got)


@pytest.mark.parametrize("cols", hx.COLS)
@pytest.mark.parametrize("exact", (False, True))
def test_pack_layout_and_unpack(cols, exact):
    ld, re = hx.pad_ld(cols), hb.row_elems(cols, exact)
    x = hb.local_values(hx.N_LOCAL, cols)
    for n in (0, 1, 7, 257):
        send = hx.send_list(n, cols)
        buf = hb.pack(x, send, cols, exact)
        assert buf.dtype == np.uint16 and buf.size == n * re
        b = buf.reshape(n, re)
        assert (b[:, cols:] == 0).all()
        assert np.array_equal(b[:, :cols], _torch_bits(x[send.astype(np.int64)]).reshape(n, cols))
        slots = hx.recv_slots(n, cols)
        ghost = np.full((n, ld), np.nan, np.float32)
        hb.unpack(ghost, slots, buf, cols, exact)
        assert not np.isnan(ghost).any()
        assert (ghost[:, cols:].view(np.uint32) == 0).all()
        want = hb.rounded(x[send.astype(np.int64)]).reshape(n, cols)
        assert np.array_equal(ghost[slots.astype(np.int64), :cols].view(np.uint32), want.view(np.uint32))
    w = hb.wire_values(5, cols, exact).reshape(5, re)
    assert (w[:, cols:] == 0).all() and not np.isnan(hb.widen(w)).any()


def test_rule():
    for gnn in (hb.GCN, hb.GAT):
        assert [hb.ships_bf16(gnn, hb.FORWARD, m) for m in (0, 1, 2)] == [False, True, True]
        assert [hb.ships_bf16(gnn, hb.BACKWARD, m) for m in (0, 1, 2)] == [False, False, True]
        assert not any(hb.ships_bf16(gnn, d, 2, switch=0) for d in (0, 1))
    assert not any(hb.ships_bf16(hb.GATMH, d, m) for d in (0, 1) for m in (0, 1, 2))


def test_peer_offsets_are_floats():
    c, o = hb.peer_offsets([0, 3, 5], 41, True)
    assert list(c) == [0, 66, 110] and list(o) == [0, 0, 66]
    c, o = hb.peer_offsets([0, 3, 5], 41, False)
    assert list(c) == [0, 96, 160] and list(o) == [0, 0, 96]
