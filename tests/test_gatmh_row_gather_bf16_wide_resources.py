"""The register budget of the wide bf16 kernels of the multi-head GAT's row-gather family (csrc/gat_mh_rows.hip,
dory_gatmh_row_gather_bf16_wide: gatmh_rows8_*_kernel), read from the code objects inside the built library as
tests/test_gatmh_row_gather_resources.py reads the family's other kernels (no GPU needed).

A wide lane keeps two float4s where a narrow lane keeps one -- twice the accumulators and twice the gathered registers of a batch of
four rows.  The condition is the family's all the same: at most 128 vector registers -- four waves per SIMD, what a latency-bound gather
lives on -- and no spills; and exactly the instantiations the launchers can select are present: lanes per row (8, 16, 32) with the
scores from the gathered row and (16, 32) with gathered scores for the forward and the destination side, (8, 16, 32) for the source
side; one-pass, hub, list and list-hub bodies for the forward and the source side, one-pass and hub for the destination side."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
EDGE = [(8, 1), (16, 1), (32, 1), (16, 0), (32, 0)]       # (lanes per row, scores from the gathered row)


def _kernels():
    lib = os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm tools missing")
    found, names = {}, []
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True,
                                   text=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", notes):
                if "gatmh_rows8_" not in m.group(1):
                    continue
                names.append(m.group(1))
                t = re.search(r"gatmh_rows8_(forward|dst|src)_(list_)?(hub_)?kernelILi(\d+)E(?:Lb([01])E)?E", m.group(1))
                if t:   # pass, list form, hub form, lanes per row, scores from the gathered row (forward, dst)
                    key = (t.group(1), bool(t.group(2)), bool(t.group(3)), int(t.group(4))) + ((int(t.group(5)),) if t.group(5) else ())
                    found[key] = (int(m.group(2)), int(m.group(3)))
    return found, names


def test_exactly_the_42_wide_instantiations_are_present_and_fit_without_spills():
    found, names = _kernels()
    want = {("forward", l, h, g, e) for g, e in EDGE for l in (False, True) for h in (False, True)}
    want |= {("dst", False, h, g, e) for g, e in EDGE for h in (False, True)}
    want |= {("src", l, h, g) for g in (8, 16, 32) for l in (False, True) for h in (False, True)}
    assert len(want) == 42
    assert set(found) == want, sorted(set(found) ^ want, key=str)
    assert len(names) == 42 and len(set(names)) == 42, names     # nothing else is named gatmh_rows8_*
    assert not [n for n in names if "gatmh_rows_" in n]          # (the family's name sets, pinned by its other resource tests, are untouched)
    for key, (vgpr, spill) in sorted(found.items(), key=str):
        print("gatmh_rows8 kernel", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)
