"""The register budget of the wide bf16 forms of the multi-head GAT sweeps (option gatmh_bf16_wide; csrc/gat_mh_sweep.hip:
gatmh_forward_sweep_bf16x8_kernel, gatmh_src_sweep_bf16x8_kernel), read from the code objects inside the built library as
tests/test_bf16_wide_resources.py reads K1s's (no GPU needed).

The forms run one 1024-thread workgroup per CU: 128 registers per lane at most, and a spilled register would be a dependent
scratch access in the chain LDS -> gathers -> sums.  The launchers select exactly one form per pass and lanes-per-head count
(D / 8 = 2, 4, 8): two rows per 16-lane group with the loader wave.  Nothing else may be instantiated, and every one has to fit."""
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
                t = re.search(r"gatmh_(forward|src)_sweep_bf16x8_kernelILi(\d+)ELi(\d+)ELb([01])EE", m.group(1))
                if t:   # pass, HL, R, LOADER
                    out[(t.group(1), int(t.group(2)), int(t.group(3)), int(t.group(4)))] = (int(m.group(2)), int(m.group(3)))
    return out


def test_every_wide_gat_instantiation_is_selectable_and_fits_without_spills():
    ks = _wide_kernels()
    # what launch_gatmh_forward_sweep_part / launch_gatmh_src_sweep_part can select: HL = D / 8 for D = 16, 32, 64; R = 2; loader on
    assert set(ks) == {(p, hl, 2, 1) for p in ("forward", "src") for hl in (2, 4, 8)}, sorted(ks)
    for key, (vgpr, spill) in sorted(ks.items()):
        print("gatmh_%s_sweep_bf16x8_kernel<HL, R, LOADER> =" % key[0], key[1:], "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)
