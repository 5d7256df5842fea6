"""The register budget of the kernels dory_gat_bf16_gather adds (csrc/spmm.hip: spmm_sweep_bf16_unit_kernel, the narrow sweep on
bf16 rows with unit weights and a row factor; spmm_sweep_bf16x8_unit_kernel, its wide form; csrc/elementwise.hip:
row_axpy_bf16_kernel), read from the code objects inside the built library as tests/test_bf16_wide_resources.py reads the
weighted wide form's (no GPU needed).

The sweeps run one 1024-thread workgroup per CU: 128 registers per lane at most, and a spilled register would be a dependent
scratch access in the chain LDS -> gathers -> sums.  The launcher can select every instantiation, so every one has to fit."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NARROW = [(32, r) for r in (2, 4, 6, 8, 10)] + [(16, r) for r in (2, 3, 4, 5, 6, 8)]     # k1s_narrow_form (csrc/spmm.hip)


@pytest.fixture(scope="module")
def kernels():
    """mangled name -> (vgprs, spilled vgprs, scratch bytes) of every gfx950 kernel in the library"""
    lib = os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm tools missing")
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True,
                                   text=True).stdout
            for blk in re.split(r"\n\s+- \.agpr_count:", notes)[1:]:
                name = re.search(r"\.name:\s+(\S+)", blk)
                vg, sp = re.search(r"\.vgpr_count:\s+(\d+)", blk), re.search(r"\.vgpr_spill_count:\s+(\d+)", blk)
                scr = re.search(r"\.private_segment_fixed_size:\s+(\d+)", blk)
                if name and vg and sp and scr:
                    out[name.group(1)] = (int(vg.group(1)), int(sp.group(1)), int(scr.group(1)))
    assert any("spmm_sweep_kernel" in n for n in out), "no kernel notes parsed"
    return out


def _check(found, expected, what):
    assert set(found) == set(expected), (what, sorted(set(expected) ^ set(found)))
    for key, (vgpr, spill, scratch) in sorted(found.items()):
        print(what, key, "vgprs", vgpr, "spilled", spill, "scratch bytes", scratch)
        assert spill == 0 and scratch == 0, (what, key, vgpr, spill, scratch)
        assert vgpr <= 128, (what, key, vgpr)


def test_every_wide_unit_instantiation_fits_without_spills(kernels):
    found = {}
    for name, res in kernels.items():
        t = re.search(r"spmm_sweep_bf16x8_unit_kernelILi(\d+)ELb([01])EE", name)
        if t:   # R, LOADER
            found[(int(t.group(1)), int(t.group(2)))] = res
    _check(found, [(r, l) for r in (2, 3, 4, 5) for l in (0, 1)], "spmm_sweep_bf16x8_unit_kernel<R, LOADER>")


def test_every_narrow_unit_instantiation_fits_without_spills(kernels):
    found = {}
    for name, res in kernels.items():
        t = re.search(r"spmm_sweep_bf16_unit_kernelILi(\d+)ELi(\d+)ELb([01])ELb([01])EE", name)
        if t:   # GROUP, R, PAIR, LOADER
            found[tuple(int(x) for x in t.groups())] = res
    _check(found, [(g, r, p, l) for g, r in NARROW for p in (0, 1) for l in (0, 1)], "spmm_sweep_bf16_unit_kernel<GROUP, R, PAIR, LOADER>")


def test_the_weighted_forms_keep_their_names(kernels):
    """the GCN kernels the A^T grad gather runs on are the instantiations from before the feature: same names, none with UNIT"""
    wide = [n for n in kernels if re.search(r"spmm_sweep_bf16x8_kernelILi\dELb[01]EE", n)]
    narrow = [n for n in kernels if re.search(r"spmm_sweep_bf16_kernelILi\d+ELi\d+ELb0ELb[01]ELb[01]EE", n)]
    assert len(wide) == 8 and len(narrow) == 4 * len(NARROW), (len(wide), len(narrow))


def test_row_axpy_bf16_kernel_exists(kernels):
    names = [n for n in kernels if "row_axpy_bf16_kernel" in n]
    assert len(names) == 1, names
    assert kernels[names[0]][1] == 0 and kernels[names[0]][2] == 0, kernels[names[0]]
