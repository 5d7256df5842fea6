"""The register budget of the wide bf16 form of K1s (option gcn_bf16_wide; csrc/spmm.hip: spmm_sweep_bf16x8_kernel), read from the code
objects inside the built library as tests/test_kernel_resources.py reads the other sweeps' (no GPU needed).

The form runs one 1024-thread workgroup per CU: 128 registers per lane at most, and a spilled register would be a dependent scratch
access in the chain LDS -> gathers -> sums.  The launcher can select every instantiation (row counts 2 .. 5, loader wave on and off),
so every one of them has to fit -- the five-row form without the loader does so with batches of three gathers."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"


def _wide_kernels():
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
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", notes):
                t = re.search(r"spmm_sweep_bf16x8_kernelILi(\d+)ELb([01])EE", m.group(1))
                if t:   # R, LOADER
                    out[(int(t.group(1)), int(t.group(2)))] = (int(m.group(2)), int(m.group(3)))
    return out


def test_every_wide_instantiation_fits_without_spills():
    ks = _wide_kernels()
    assert set(ks) == {(r, l) for r in (2, 3, 4, 5) for l in (0, 1)}, sorted(ks)      # four row counts x loader on / off
    assert len(ks) >= 8
    for key, (vgpr, spill) in sorted(ks.items()):
        print("spmm_sweep_bf16x8_kernel<R, LOADER> =", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)
