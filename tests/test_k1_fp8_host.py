"""dory_k1_fp8_gather without a GPU (include/dorylus_hip.h): the number format as the host function states it (k1_fp8_rows) against a
numpy / torch.float8_e4m3fn statement of the definition, byte for byte and exponent for exponent; the form rule (k1_fp8_form); and
the new kernels of csrc/spmm_fp8.hip, read from the code objects inside the built library: exactly the forms of the rule, no spills,
at most 128 vector registers."""
import re

import numpy as np
import pytest

from test_gemm_bf16_host import kernels  # noqa: F401  (the fixture: {kernel name: (vector registers, spilled)})

E_MIN, E_MAX = -117, 119      # DORY_K1_FP8_EXP_MIN / _MAX


def definition(x, ld):
    """e = clamp(floor(log2 amax) - 7), 0 for a zero row; q = RNE_E4M3(clip(x 2^-e, +-448)); zero bytes in [cols, ld)"""
    import torch
    x = np.asarray(x, np.float32)
    amax = np.abs(x).max(axis=1)
    k = np.frexp(amax)[1].astype(np.int64)                       # amax = f 2^k, f in [0.5, 1)
    e = np.where(amax > 0, np.clip(k - 1 - 7, E_MIN, E_MAX), 0)
    y = np.clip(np.ldexp(x.astype(np.float64), -e[:, None]).astype(np.float32), -448, 448)
    q = np.zeros((x.shape[0], ld), np.uint8)
    q[:, :x.shape[1]] = torch.from_numpy(y).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    return q, (e + 127).astype(np.uint8)


def rows_of(cols):
    """the rows the issue lists, `cols` wide: zero, a spike among zeros, maxima at 2^k and just below 2^(k+1), rounding ties, the
    subnormal range of the scaled row, magnitudes from 1e-30 to 1e30"""
    rng = np.random.default_rng([91, cols])
    rows = [np.zeros(cols), np.eye(1, cols, cols // 2)[0] * -3.7]
    for k in (-100, -20, -1, 0, 1, 7, 33, 99):
        for top in (np.float32(2.0) ** k, np.nextafter(np.float32(2.0) ** (k + 1), np.float32(0))):
            r = rng.uniform(-1, 1, cols) * float(top)
            r[rng.integers(0, cols)] = top * rng.choice([-1.0, 1.0])
            rows.append(r)
    # maximum 1 -> e = -7, y = 128 x: ties of the binades [16, 32) (step 2), [1, 2) (step 1/8), of the subnormals (step 2^-9, below
    # 2^-6), and the values next to each tie
    ties = np.concatenate([np.arange(17, 32, 2), 1 + (2 * np.arange(8) + 1) / 16, (2 * np.arange(9) + 1) * 2.0 ** -10]) / 128
    near = np.concatenate([np.nextafter(ties.astype(np.float32), np.float32(0)), np.nextafter(ties.astype(np.float32), np.float32(1))])
    for vals in (ties, -ties, near, rng.uniform(0, 2.0 ** -6, 64) / 128):
        r = np.resize(vals, cols).astype(np.float64)
        r[0] = 1.0
        rows.append(r)
    mags = 10.0 ** rng.uniform(-30, 30, 24)
    rows += [rng.standard_normal(cols) * m for m in mags]
    rows += [rng.standard_normal(cols) * 10.0 ** rng.uniform(-30, 30, cols) for _ in range(4)]      # every magnitude in one row
    return np.asarray(rows).astype(np.float32)


@pytest.mark.parametrize("cols", [1, 41, 64, 300, 602])
def test_rows_equal_the_definition_byte_for_byte(cols):
    import dorylus_amd as da
    import aggregate_ref as ar
    x, ld = rows_of(cols), ar.pad_ld(cols)
    q, e = da.k1_fp8_rows(x, ld)
    wq, we = definition(x, ld)
    assert q.shape == (len(x), ld) and np.array_equal(e, we), np.nonzero(e != we)[0][:8]
    bad = np.argwhere(q != wq)
    assert bad.size == 0, (cols, bad[:4].tolist(), [(x[i, j], q[i, j], wq[i, j]) for i, j in bad[:4]])
    assert (q & 0x7F).max() <= 0x78 and e[0] == 127                  # nothing above 256, nothing non-finite; the zero row's e = 0
    import torch
    deq = torch.from_numpy(q[:, :cols].copy()).view(torch.float8_e4m3fn).to(torch.float64).numpy() * 2.0 ** (e.astype(np.float64) - 127)[:, None]
    assert (np.abs(deq - x) <= 2.0 ** -4 * np.abs(x).max(axis=1, keepdims=True)).all()     # each element moves by at most 2^-4 of the maximum
    assert (deq.astype(np.float32).astype(np.float64) == deq).all()                        # q 2^e is exact in fp32


@pytest.mark.parametrize("ld,slab,want", [(32, 0, None), (64, 0, (8, 1, 8)), (96, 0, (16, 1, 8)), (128, 0, (8, 1, 16)),
                                          (320, 0, (32, 1, 16)), (608, 0, (64, 1, 16)), (2048, 0, (64, 2, 16)), (2080, 0, (64, 2, 16)),
                                          (608, 256, (16, 1, 16)), (608, 64, (8, 1, 8)), (608, 32, None), (72, 0, None)])
def test_form_table(ld, slab, want):
    import dorylus_amd as da
    assert da.k1_fp8_form(ld, slab) == want


def test_the_kernels_are_the_forms_of_the_rule_and_fit_without_spills(kernels):  # noqa: F811
    import dorylus_amd as da
    gather = {}
    for name, res in kernels.items():
        t = re.search(r"k1_fp8_rows_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", name)
        if t:
            gather[tuple(int(v) for v in t.groups())] = res
    rule = {da.k1_fp8_form(ld, slab) for ld in range(32, 4200, 32) for slab in (0, 64, 96, 128, 256, 1024)} - {None}
    assert set(gather) == rule and len(rule) == 7, (sorted(gather), sorted(rule))
    others = {n: r for n, r in kernels.items() if "fp8" in n and "k1_fp8_rows_kernel" not in n}
    assert sum("k1_fp8_longrow_kernel" in n for n in others) == 1 and sum("k1_fp8_longrow_reduce_kernel" in n for n in others) == 1
    assert sum("fp8_rows_kernel" in n for n in others) == 6 and sum("fp8_rows_wide_kernel" in n for n in others) == 1 and len(others) == 9
    for name, (vgpr, spill) in sorted({**{str(k): v for k, v in gather.items()}, **others}.items()):
        print(name, "vgprs", vgpr, "spilled", spill)
        assert spill == 0 and vgpr <= 128, (name, vgpr, spill)
