"""Register budget of the bf16-row aggregation kernels (option gcn_bf16_gather), read from the code objects inside the built
library as tests/test_kernel_resources.py reads the fp32 ones (no GPU needed).  The bf16 sweeps run on the same one
1024-thread workgroup per CU: every variant stays at 128 registers or fewer, and the variants the launcher selects by
default (sweep_rows, the loader wave on 32-lane launches) do not spill."""
from test_kernel_resources import _kernels, _tparams


def test_bf16_sweep_variants_fit_and_default_ones_do_not_spill():
    ks = _kernels()
    seen, bad = 0, []
    for name, (vgpr, spill) in ks.items():
        p = _tparams(name, "spmm_sweep_bf16_kernel")
        if not p:
            continue
        group, r, unit, pair, loader = p
        assert vgpr <= 128, (name, vgpr)
        assert unit == 0, name                     # bf16 rows: edge weights only (GCN), no unit-weight form
        default = (group == 32 and loader == 1) or (group == 16 and pair == 0 and r <= 6)
        if default:
            seen += 1
            if spill:
                bad.append((name, vgpr, spill))
    assert seen >= 10, seen
    assert not bad, bad


def test_bf16_row_gather_kernels_do_not_spill():
    ks = _kernels()
    names = [n for n in ks if any(s in n for s in ("spmm_rows_bf16_kernel", "spmm_longrow_bf16_kernel",
                                                    "spmm_sweep_combine_bf16_kernel", "bf16_rows_kernel"))]
    assert len([n for n in names if "spmm_rows_bf16_kernel" in n]) == 8, names
    assert any("spmm_longrow_bf16_kernel" in n for n in names) and any("spmm_sweep_combine_bf16_kernel" in n for n in names)
    assert any("bf16_rows_kernel" in n and "spmm" not in n for n in names), names
    for n in names:
        vgpr, spill = ks[n]
        assert spill == 0, (n, vgpr, spill)
