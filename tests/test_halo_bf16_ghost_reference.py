"""tests/halo_bf16_ghost_ref.py against torch on the CPU (no GPU): the widening is torch's bf16 -> fp32 on the bit patterns of
tests/halo_bf16_ref.py (ties, denormals, +-0, +-FLT_MAX -> inf, +-inf); the keep form writes the wire rows at the listed twin rows
with zeros in [row_elems, ld) whatever the twin held; and the identity the feature rests on: the twin after keep is the rounding of
the fp32 ghost rows the widening unpack of dory_halo_bf16_rows leaves, and widening it gives those rows back -- for every width of
halo_exact_ref.COLS with a twin (ld >= 4), padded and exact rows.  The wire rule and the direct landing."""
import numpy as np
import pytest

import halo_bf16_ghost_ref as hg
import halo_bf16_ref as hb
import halo_exact_ref as hx

TWIN_COLS = [c for c in hx.COLS if hx.pad_ld(c) >= 4]


def _torch_widen(u16):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(u16, np.uint16).view(np.int16)).view(torch.bfloat16)
    return t.to(torch.float32).numpy()


def test_widening_is_torchs_on_the_bit_patterns():
    x = np.concatenate([hb.patterns(100000, seed=11), hb.named_patterns().view(np.float32)])
    b = hb.round_bits(x)
    got, want = hg.widen(b), _torch_widen(b)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got.view(np.uint32), hb.rounded(x).view(np.uint32))
    for name in ("tie_down_to_even", "tie_up_to_even", "denormal_big", "minus_zero", "flt_max", "minus_flt_max", "plus_inf", "minus_inf"):
        u = np.array([hb.NAMED[name]], np.uint32).view(np.float32)
        assert hg.widen(hb.round_bits(u)).view(np.uint32)[0] == _torch_widen(hb.round_bits(u)).view(np.uint32)[0], name
    assert hg.widen(np.array([0x8000], np.uint16)).view(np.uint32)[0] == 0x80000000      # -0 keeps its sign
    assert np.isposinf(hg.widen(hb.round_bits(np.array([0x7F7FFFFF], np.uint32).view(np.float32)))[0])


def test_twin_widths():
    assert TWIN_COLS == [3, 5, 6, 20, 25, 32, 33, 41, 63, 602] and hx.pad_ld(1) == 1
    for cols in TWIN_COLS:
        assert hx.pad_ld(cols) % 32 == 0 and hb.row_elems(cols, True) <= hb.row_elems(cols, False) == hx.pad_ld(cols)


@pytest.mark.parametrize("cols", TWIN_COLS)
@pytest.mark.parametrize("exact", (False, True))
def test_keep_is_the_rounding_of_the_fp32_unpack(cols, exact):
    ld, re = hx.pad_ld(cols), hb.row_elems(cols, exact)
    for n in (0, 1, 3, 257):
        slots = hx.recv_slots(n, cols)
        wire = hb.wire_values(n, cols, exact)
        twin = np.full((n, ld), 0x7FC0, np.uint16)                 # poisoned: bf16 NaN everywhere
        hg.keep(twin, slots, wire, cols, exact)
        assert (twin[:, re:] == 0).all() and (twin[:, cols:] == 0).all()
        assert np.array_equal(twin[slots.astype(np.int64), :re], wire.reshape(n, re))
        fp32 = hb.unpack(np.full((n, ld), np.nan, np.float32), slots, wire, cols, exact)      # what dory_halo_bf16_rows alone leaves
        assert np.array_equal(twin, hb.round_bits(fp32)), (cols, exact, n, "keep == round(unpack_fp32)")
        assert np.array_equal(hg.widen(twin).view(np.uint32), fp32.view(np.uint32)), (cols, exact, n, "widen(keep) == unpack_fp32")
        assert np.array_equal(hg.widen(twin).view(np.uint32), _torch_widen(twin).view(np.uint32))


def test_keep_of_packed_named_patterns_round_trips():
    """pack (rounding) -> keep -> widen is the rounding of the owner's rows, named cases included"""
    cols = 41
    x = hb.local_values(hx.N_LOCAL, cols)
    send = hx.send_list(257, cols)
    for exact in (False, True):
        buf = hb.pack(x, send, cols, exact)
        twin = hg.keep(np.full((257, 64), 0xFFFF, np.uint16), np.arange(257), buf, cols, exact)
        assert np.array_equal(hg.widen(twin)[:, :cols].view(np.uint32), hb.rounded(x[send.astype(np.int64)]).view(np.uint32))
        assert (twin[:, cols:] == 0).all()


def test_wire_rule_and_direct_landing():
    for gnn in (hb.GCN, hb.GAT):
        for d, m in ((hb.FORWARD, 1), (hb.FORWARD, 2), (hb.BACKWARD, 2)):
            assert hg.wire_bf16(gnn, d, m, 1, 0, False, 41) and hg.wire_bf16(gnn, d, m, 1, 1, False, 41)
            assert not hg.wire_bf16(gnn, d, m, 1, 0, True, 41) and hg.wire_bf16(gnn, d, m, 1, 1, True, 41)
            assert not hg.wire_bf16(gnn, d, m, 1, 1, True, 1)            # a one-column tensor has no twin: a direct plan keeps fp32
            assert hg.wire_bf16(gnn, d, m, 1, 1, False, 1)               # ... a staged one ships bf16 into the widening unpack as before
            assert not hg.wire_bf16(gnn, d, m, 0, 1, True, 41) and not hg.wire_bf16(gnn, d, m, 1, 1, True, 41, scatter=True)
        assert not hg.wire_bf16(gnn, hb.BACKWARD, 1, 1, 1, True, 41)
    assert not any(hg.wire_bf16(hb.GATMH, d, 2, 1, 1, dp, 128) for d in (0, 1) for dp in (False, True))
    assert hg.lands_directly(True, 41, False) and not hg.lands_directly(True, 41, True) and not hg.lands_directly(False, 41, False)
    assert hg.lands_directly(True, 32, True) and hg.lands_directly(True, 602, False) and not hg.lands_directly(True, 602, True)
