"""CPU-only: dory_gatmh_bf16_ghosts (include/dorylus_hip.h) is exported and bound, and the numpy mirror of the keep form of the merged
unpack (tests/gatmh_bf16_ghost_ref.py) agrees with today's unpack (tests/gatmh_halo_bf16_ref.py: the do part widened into bg_do's fp32
rows) followed by a rounding of those rows -- widening and rounding a bf16 cancel, and zeros stay zeros."""
import ctypes
import os

import numpy as np
import pytest

import gatmh_bf16_ghost_ref as gg
import gatmh_halo_bf16_ref as gr
import halo_bf16_ref as hb


def test_library_exports_and_context_binds_the_switch_and_its_counters():
    import dorylus_amd
    assert os.path.exists(dorylus_amd.LIB_PATH), "the library is not built"
    lib = ctypes.CDLL(dorylus_amd.LIB_PATH)
    for s in ("dory_gatmh_bf16_ghosts", "dory_gatmh_bf16_ghosts_stats"):
        assert hasattr(lib, s) and s in dorylus_amd.SYMBOLS, s
    assert callable(dorylus_amd.Context.gatmh_bf16_ghosts) and callable(dorylus_amd.Context.gatmh_bf16_ghosts_stats)
    assert len(dorylus_amd.Context.GATMH_BF16_GHOSTS_STATS) == 7


@pytest.mark.parametrize("K", [1, 3, 8, 32])
@pytest.mark.parametrize("w", [8, 24, 48, 128])
def test_keep_form_is_the_widening_unpack_followed_by_a_rounding(w, K):
    rng = np.random.default_rng([w, K])
    G, n = 9, 7                                             # two ghost rows no list names; a slot order that is no identity
    ld, ld_st = gr.pad_ld(w), gr.pad_ld(4 * K)
    cols = w - 3 if w > 8 else w                            # (exact rows: zeros stand behind cols up to w)
    do = hb.local_values(n, cols, salt=K)                   # bit patterns without NaN, ties and binade edges among them
    st = rng.uniform(0.5, 1.5, (n, 4 * K)).astype(np.float32)
    buf = gr.pack(do, st, K, w, [np.arange(n)])
    lists = [[], list(rng.permutation(G)[:n])]
    old_do = rng.standard_normal((G, ld)).astype(np.float32)
    old_st = rng.standard_normal((G, ld_st)).astype(np.float32)
    want_do, want_st = gr.unpack(buf, K, w, lists, G, ld, ld_st, bg_do=old_do, bg_st=old_st)
    twin, got_st = gg.unpack_keep(buf, K, w, lists, G, ld, ld_st, twin=hb.round_bits(old_do), bg_st=old_st)
    assert np.array_equal(twin, hb.round_bits(want_do))
    assert np.array_equal(got_st.view(np.uint32), want_st.view(np.uint32))
    named = np.asarray(lists[1], np.int64)
    assert (twin[named, w:] == 0).all() and (twin[named, cols:w] == 0).all()
    assert np.array_equal(hb.widen(twin[named]).view(np.uint32), want_do[named].view(np.uint32))     # (nothing is lost either way)
    # without given arrays the rows no list names are marked
    twin2, st2 = gg.unpack_keep(buf, K, w, lists, G, ld, ld_st)
    rest = np.setdiff1d(np.arange(G), named)
    assert (twin2[rest] == 0x7FC1).all() and np.isnan(st2[rest]).all() and np.array_equal(twin2[named], twin[named])
