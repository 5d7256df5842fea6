"""The shape rule of the wide (16-byte) bf16 form of the multi-head GAT's row-gather kernels (dory_gatmh_row_gather_bf16_wide;
csrc/gat_mh_shapes.hpp: gatmh_rows8_form), asked through dory_gatmh_row_gather_bf16_wide_form (include/dorylus_host.h): no context,
no GPU.  The launchers of csrc/gat_mh_rows.hip select their instantiation by the same function.

Taken where the family covers the shape, 64 <= ld <= 256, and K == 1 or D % 8 == 0: lanes per row 8 / 16 / 32 for ld / 8 <= 8, <= 16,
more; lanes per head the row's lanes for one head, else D / 8; the scores come from the gathered row where ld / 4 is a power of two."""
import pytest

TAKEN = [   # (K, D, ld) -> (lanes per row, lanes per head, scores from the gathered row)
    ((8, 8, 64), (8, 1, True)), ((4, 16, 64), (8, 2, True)), ((1, 41, 64), (8, 8, True)),
    ((8, 16, 128), (16, 2, True)), ((2, 64, 128), (16, 8, True)), ((1, 100, 128), (16, 16, True)),
    ((32, 8, 256), (32, 1, True)), ((4, 64, 256), (32, 8, True)), ((1, 256, 256), (32, 32, True)),
    ((3, 32, 96), (16, 4, False)), ((5, 32, 160), (32, 4, False)), ((1, 200, 224), (32, 32, False)),
]
NOT_TAKEN = [(4, 2, 32), (8, 4, 32), (16, 4, 64), (32, 2, 64), (32, 1, 32), (1, 6, 32),
             (1, 8, 288), (8, 32, 288),          # rows past 256 floats: the family refuses them
             (8, 16, 64), (2, 64, 96),           # K*D > ld
             (3, 24, 96), (0, 8, 64), (8, 0, 64), (65, 1, 128), (1, 8, 0), (1, 8, 66)]   # no shape of the model / of the family


@pytest.fixture(scope="module")
def form():
    import dorylus_amd
    return dorylus_amd.gatmh_row_gather_bf16_wide_form


@pytest.mark.parametrize("shape,want", TAKEN)
def test_shapes_that_take_the_wide_form(form, shape, want):
    assert form(*shape) == want, (shape, form(*shape))


@pytest.mark.parametrize("shape", NOT_TAKEN)
def test_shapes_that_stay_narrow(form, shape):
    assert form(*shape) is None, (shape, form(*shape))


def test_the_rule_over_every_row_width(form):
    """every ld the model pads rows to (multiples of 32) and every head shape: the three conditions, the geometry, and nothing else"""
    for ld in range(32, 321, 32):
        for K in (1, 2, 3, 4, 5, 8, 16, 32, 64):
            for D in (1, 2, 4, 6, 8, 16, 32, 41, 64, 100, 200, 256):
                shape_ok = K * D <= 256 and (K == 1 or (D & (D - 1) == 0 and D <= 64))
                rows_ok = shape_ok and ld <= 256 and K * D <= ld
                want = rows_ok and ld >= 64 and (K == 1 or D % 8 == 0)
                got = form(K, D, ld)
                assert (got is not None) == want, (K, D, ld, got)
                if got:
                    n8, n4 = ld // 8, ld // 4
                    lanes = 8 if n8 <= 8 else 16 if n8 <= 16 else 32
                    assert got == (lanes, lanes if K == 1 else D // 8, n4 & (n4 - 1) == 0), (K, D, ld, got)
                    assert lanes * 8 >= ld and got[1] & (got[1] - 1) == 0      # the row fits its lanes; a head's lanes are a butterfly


def test_null_outputs_and_zeroed_outputs():
    import ctypes as C
    import dorylus_amd
    lib = dorylus_amd.load()
    assert lib.dory_gatmh_row_gather_bf16_wide_form(8, 16, 128, None, None, None) == 1
    lr, lh, el = C.c_uint32(7), C.c_uint32(7), C.c_int32(7)
    assert lib.dory_gatmh_row_gather_bf16_wide_form(4, 2, 32, C.byref(lr), C.byref(lh), C.byref(el)) == 0
    assert (lr.value, lh.value, el.value) == (0, 0, 0)
