"""The dot-product argument of the wide bf16 form of the multi-head GAT's row-gather kernels (csrc/gat_mh_rows.hip,
dory_gatmh_row_gather_bf16_wide), restated in numpy float32: no GPU, no kernels -- the written proof the bit test of
tests/test_gpu_gatmh_row_gather_bf16_wide.py relies on.

The narrow form reduces a head's dot product over HL lanes: every lane forms a four-term fmaf chain over its float4, then
rows_allreduce runs a butterfly -- quad_perm [1,0,3,2], quad_perm [2,3,0,1], row_half_mirror, row_mirror, xor 16, xor 32 -- in which
every lane adds its partner's value to its own.  The wide form keeps two float4s a lane: it forms the same two chains, adds them inside
the lane, and runs the same butterfly over HL / 2 lanes.  Claim: every lane of the wide form holds the bits every lane of the narrow
form holds.  Why: the in-lane sum a + b is what the narrow lanes 2j and 2j + 1 hold after the first step (a + b and b + a: IEEE addition
commutes), and from there on wide lane j and narrow lanes 2j, 2j + 1 add the same partners' values in the same order; the mirrors hand
over the value of a lane in the other half of the 8 / 16 lanes, all of whose lanes agree by then."""
import numpy as np
import pytest

F = np.float32


def fma(a, b, c):
    """a * b + c rounded once (the product of two float32 is exact in float64; the float64 sum is the value rounded here)"""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(F)


def chain(x, y):
    """rows_dot's chain over a float4: fmaf(x0, y0, fmaf(x1, y1, fmaf(x2, y2, x3 * y3))); x, y: [lanes, 4]"""
    return fma(x[:, 0], y[:, 0], fma(x[:, 1], y[:, 1], fma(x[:, 2], y[:, 2], (x[:, 3] * y[:, 3]).astype(F))))


def chain_el(x, y):
    """rows_el's chain: fmaf(x3, y3, fmaf(x2, y2, fmaf(x1, y1, fmaf(x0, y0, 0))))"""
    z = np.zeros(x.shape[0], F)
    return fma(x[:, 3], y[:, 3], fma(x[:, 2], y[:, 2], fma(x[:, 1], y[:, 1], fma(x[:, 0], y[:, 0], z))))


def allreduce(v, HL):
    """rows_allreduce over aligned runs of HL lanes of a 64-lane wave: the moves of the kernel, lane by lane"""
    v = v.astype(F).copy()
    lane = np.arange(64)
    steps = [(1, lane ^ 1), (2, lane ^ 2), (4, (lane & ~7) | (7 - (lane & 7))), (8, (lane & ~15) | (15 - (lane & 15))),
             (16, lane ^ 16), (32, lane ^ 32)]
    for width, partner in steps:
        if HL > width:
            v = (v + v[partner]).astype(F)
    return v


def rows(rng, HL, dead):
    """two operand rows for a wave of 64 narrow lanes: magnitudes over many binades, negatives, zeros; `dead` lanes at the end of
    every run of HL lanes contribute zero (masked operand), as lanes past the row or past K*D do"""
    x = (rng.standard_normal((64, 4)) * np.exp2(rng.integers(-20, 20, (64, 4)))).astype(F)
    y = (rng.standard_normal((64, 4)) * np.exp2(rng.integers(-6, 6, (64, 4)))).astype(F)
    x[rng.random((64, 4)) < 0.15] = 0
    y[rng.random((64, 4)) < 0.1] = 0
    if dead:
        y[(np.arange(64) % HL) >= HL - dead] = 0
    return x, y


@pytest.mark.parametrize("make_chain", [chain, chain_el], ids=["rows_dot", "rows_el"])
@pytest.mark.parametrize("HL", [2, 4, 8, 16, 32, 64])
def test_in_lane_add_then_half_butterfly_gives_the_narrow_bits(HL, make_chain):
    rng = np.random.default_rng(HL)
    for trial in range(200):
        dead = 0 if trial % 3 == 0 else int(rng.integers(0, HL))
        x, y = rows(rng, HL, dead)
        c = make_chain(x, y)                                  # the narrow lanes' chains; wide lane j forms c[2j] and c[2j + 1]
        narrow = allreduce(c, HL)
        w = np.zeros(64, F)
        w[:32] = (c[0::2] + c[1::2]).astype(F)                # the in-lane add; 32 wide lanes stand for the 64 narrow ones
        wide = allreduce(w, HL // 2)
        assert np.array_equal(wide[:32].view(np.uint32), narrow[0::2].view(np.uint32)), (HL, trial, dead)
        assert np.array_equal(wide[:32].view(np.uint32), narrow[1::2].view(np.uint32)), (HL, trial, dead)
        # every lane of a head agrees, and a head is an aligned run of HL lanes
        heads = narrow.reshape(-1, HL).view(np.uint32)
        assert np.array_equal(heads, np.repeat(heads[:, :1], HL, 1)), (HL, trial)


def test_the_mirrors_are_the_xor_partners_once_the_quads_agree():
    """row_half_mirror / row_mirror read lane 7 - i / 15 - i: after the quad steps that lane holds what lane i ^ 4 / i ^ 8 holds"""
    rng = np.random.default_rng(0)
    c = rng.standard_normal(64).astype(F)
    for HL in (8, 16, 32, 64):
        v = c.copy()
        lane = np.arange(64)
        off = 1
        while off < HL:
            v = (v + v[lane ^ off]).astype(F)
            off *= 2
        assert np.array_equal(v.view(np.uint32), allreduce(c, HL).view(np.uint32)), HL


def test_a_head_of_eight_features_needs_no_lane_step():
    """D == 8: the narrow head is two lanes (one butterfly step), the wide head one lane -- the in-lane add is the whole reduction"""
    rng = np.random.default_rng(1)
    x, y = rows(rng, 2, 0)
    c = chain(x, y)
    assert np.array_equal(allreduce(c, 2)[0::2].view(np.uint32), (c[0::2] + c[1::2]).astype(F).view(np.uint32))
