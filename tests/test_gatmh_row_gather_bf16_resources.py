"""The register budget of the bf16 forms of the multi-head GAT's row-gather kernels (csrc/gat_mh_rows.hip; dory_gatmh_row_gather_bf16),
read from the code objects inside the built library as tests/test_gatmh_row_gather_resources.py reads their fp32 siblings (no GPU needed).

The bf16 kernels share their siblings' bodies; what differs is the gathered chunk: one 8-byte load of four bf16, widened in registers.
The condition is the siblings', for the siblings' reason -- HBM-latency-bound gathers live on resident waves, and 128 vector registers
are four waves per SIMD -- together with: no spills, and every instantiation the launchers can select is present (the same 31 forms)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FORMS = [(g, 1) for g in (8, 16, 32, 64)] + [(g, 2) for g in (8, 16, 32)] + [(g, 4) for g in (8, 16)]


def _kernels():
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
                t = re.search(r"gatmh_rows_(forward|dst|src)_bf16_kernelILi(\d+)ELi(\d+)E(?:Li(\d+)E|Lb([01])E)E", m.group(1))
                if t:   # pass, GROUP, HPQ, rows in flight (source side) or scores from the gathered row (forward, destination side)
                    key = (t.group(1), int(t.group(2)), int(t.group(3)), int(t.group(4) if t.group(4) else t.group(5)))
                    out[key] = (int(m.group(2)), int(m.group(3)))
    return out


def test_every_bf16_row_gather_instantiation_is_present_and_fits_without_spills():
    ks = _kernels()
    edge = [(g, h, 1) for g, h in FORMS] + [(32, 1, 0), (64, 1, 0)]     # (rows of 96, 160, 192, 224 floats gather their scores)
    want = {("forward",) + f for f in edge} | {("dst",) + f for f in edge} | {("src", g, h, 2 if h == 4 else 4) for g, h in FORMS}
    assert set(ks) == want, sorted(set(ks) ^ want)
    assert len(ks) == 31
    for key, (vgpr, spill) in sorted(ks.items()):
        print("gatmh_rows bf16 kernel", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)
