"""The host arithmetic of a launch on the sweep skeleton (dorylus_amd/host/sweep_geometry.cpp, used by the launchers in
csrc/spmm.hip and csrc/gat_mh_sweep.hip and by the callers that size the gate counters), through dory_sweep_geometry.
No GPU.  The reference is the tests' mirror (aggregate_ref.py: sweep_pick_r, sweep_rows_for, the geometry lines of dispatch)."""
import ctypes as C
import itertools

import numpy as np
import pytest

import aggregate_ref as ar
from dorylus_amd import _lib as L

NS = (8, 9, 2047, 33000, 70001, 232965)
GROUPS = (16, 32)
CUS = (1, 4, 12, 13, 28, 32)
OPTIONS = (0, 2, 3, 4, 5, 6, 7, 8, 10)
LDS = (32, 64, 96, 128, 256, 608)
RESERVES = (0, 4, 8, 20)
NB = 5
SLABS, RPX, TILES_X, SPP, NSWEEPS, GRID_X, BLOCK_WORDS, CLEARED, BOUND, RULE_R, WIDE_ROWS = range(11)


def _cdiv(a, b):
    return -(-a // b)


@pytest.fixture(scope="module")
def lib():
    return L.load()


def _hook(lib, npos, ld, group, rows, wide, cus, nblocks, layout_rows, option):
    out = np.zeros(11, np.uint64)
    rc = lib.dory_sweep_geometry(npos, ld, group, rows, int(wide), cus, nblocks, layout_rows, option, out.ctypes.data_as(C.c_void_p))
    return rc, [int(x) for x in out]


def _npos(lib, cache, N, Rl, G):
    if (N, Rl, G) not in cache:
        npos = C.c_uint32(0)
        assert lib.dory_sweep_deal(N, Rl, G, C.byref(npos), None, None) == 0
        cache[(N, Rl, G)] = npos.value
    return cache[(N, Rl, G)]


def _mirror(npos, ld, group, R, wide, G):
    """aggregate_ref.dispatch's geometry lines; the wide form: 16-lane groups on chunks of eight features"""
    if wide:
        group = 16
    RW = ar.SWEEP_NT // group * R
    rpx = _cdiv(_cdiv(npos, 8), R) * R
    tiles_x = _cdiv(rpx, RW)
    slabs = _cdiv(ld // (8 if wide else 4), group)
    return slabs, rpx, tiles_x, _cdiv(tiles_x, G)


def _parent_bound_words(npos, ld, group, R, wide, G, nblocks):
    """sweep_scratch_bytes of commit 5e9da16, in words: slack constants of its own"""
    if wide:
        group = 16
    RW = ar.SWEEP_NT // group * R
    Gmin = G - 8 if G > 12 else G
    rpx = (npos + 7) // 8 + 16
    tiles = _cdiv(rpx, RW) + 1
    spp = _cdiv(tiles, Gmin)
    slabs = _cdiv(ld >> (3 if wide else 2), group)
    return 8 * slabs * spp * nblocks * 32 + 1


def test_grid_against_the_mirror_and_the_counter_bound(lib):
    cache, walked, wide_walked = {}, 0, 0
    for N, group, G, option, ld, wide in itertools.product(NS, GROUPS, CUS, OPTIONS, LDS, (False, True)):
        Rl = ar.sweep_pick_r(N, 32, G, option)                  # the layout is dealt for the 32-lane launches
        npos = _npos(lib, cache, N, Rl, G)
        R = ar.sweep_rows_for(Rl, 16 if wide else group, G, option)
        R16 = ar.sweep_rows_for(Rl, 16, G, option)
        if wide and not (ld >= 128 and 2 <= R16 <= 5):          # no wide launch of this shape
            continue
        rc, o = _hook(lib, npos, ld, group, R, wide, G, NB, Rl, option)
        assert rc == 0
        key = (N, group, G, option, ld, wide)
        # 1. the rule's R and the geometry equal the mirror
        assert o[RULE_R] == R, key
        assert o[WIDE_ROWS] == int(2 <= R16 <= 5), key
        slabs, rpx, tiles_x, spp = _mirror(npos, ld, group, R, wide, G)
        assert (o[SLABS], o[RPX], o[TILES_X], o[SPP]) == (slabs, rpx, tiles_x, spp), key
        assert o[NSWEEPS] == slabs * spp and o[GRID_X] == 8 * slabs * spp * G and o[BLOCK_WORDS] == 8 * slabs * spp * 32, key
        assert o[CLEARED] == o[BLOCK_WORDS] * NB + 1, key
        # 2. whatever a launch leaves to concurrent kernels and whichever blocks it walks, it clears no more than the bound
        for reserve in RESERVES:
            Gl = G - min(reserve, 8) if G > 12 else G           # (sweep_plan)
            rc, q = _hook(lib, npos, ld, group, R, wide, Gl, NB, Rl, option)
            assert rc == 0 and q[CLEARED] <= o[BOUND], (key, reserve)
            assert q[BOUND] >= q[CLEARED]
            for b_lo, b_hi in itertools.combinations(range(NB + 1), 2):
                assert q[BLOCK_WORDS] * (b_hi - b_lo) + 1 <= o[BOUND], (key, reserve, b_lo, b_hi)
        # 3. ... and the bound never exceeds the parent's
        assert o[BOUND] <= _parent_bound_words(npos, ld, group, R, wide, G, NB), key
        walked += 1
        wide_walked += wide
    assert walked > 3000 and wide_walked > 500, (walked, wide_walked)


def test_the_hook_takes_rows_never_an_option(lib):
    """4. an actual row count is used as given: seven rows (as an option: valid for no lane-group width) are seven rows, the
    GAT passes' two rows are two rows whatever option spmm_sweep_rows says, and "0 = pick" does not exist"""
    npos = 8 * 2 * 1024 * 8
    rc, o = _hook(lib, npos, 128, 32, 7, False, 32, 1, 8, 0)
    assert rc == 0 and o[RPX] == _cdiv(npos // 8, 7) * 7 and o[TILES_X] == _cdiv(o[RPX], 32 * 7)
    for option in OPTIONS:
        rc, o = _hook(lib, npos, 128, 32, 2, False, 32, 1, 8, option)
        assert rc == 0 and (o[RPX], o[TILES_X]) == (npos // 8, npos // 8 // 64), option
    assert _hook(lib, npos, 128, 32, 0, False, 32, 1, 8, 0)[0] != 0
    assert _hook(lib, npos, 128, 32, -1, False, 32, 1, 8, 0)[0] != 0


def test_forced_rows_are_honoured_where_they_have_kernels(lib):
    npos = 8 * 2 * 1024 * 8

    def rule(group, layout_rows, option):
        rc, o = _hook(lib, npos, 128, group, 2, False, 32, 1, layout_rows, option)
        assert rc == 0
        return o[RULE_R]
    for layout_rows in (2, 4, 6, 8, 10):
        # 5. option 7 is valid for no group: as with 0
        assert [rule(g, layout_rows, 7) for g in GROUPS] == [rule(g, layout_rows, 0) for g in GROUPS] == [max(2, layout_rows // 2), layout_rows]
    # 6. 3 and 5 on 16 lanes and only there, 10 on 32 lanes and only there (a layout of eight rows: 4 and 8 rows unforced)
    assert [rule(16, 8, f) for f in (3, 5, 10)] == [3, 5, 4]
    assert [rule(32, 8, f) for f in (3, 5, 10)] == [8, 8, 10]
    for f in (2, 4, 6, 8):
        assert rule(16, 10, f) == f and rule(32, 10, f) == f
