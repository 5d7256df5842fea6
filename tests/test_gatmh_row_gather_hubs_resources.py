"""The register budget of the hub-splitting kernels of the multi-head GAT's row-gather family (csrc/gat_mh_rows.hip,
dory_gatmh_row_gather_hub_split), read from the code objects inside the built library as tests/test_gatmh_row_gather_resources.py reads
the family's one-pass kernels (no GPU needed).

A split pass launches the *_hub_kernel of the pass (the chunks of the hub rows and the rows that are no hub rows: the one-pass body with
an entry range) and its *_merge_kernel (one lane group per hub row).  The condition is the family's: at most 128 vector registers -- four
waves per SIMD, what a latency-bound gather lives on -- no spills, and every instantiation the launchers can select present, in fp32 and
bf16: the forms of the one-pass kernels for the hub kernels, (lane group, heads per float4) for the merge kernels."""
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
    hub, merge = {}, {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True,
                                   text=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", notes):
                t = re.search(r"gatmh_rows_(forward|dst|src)_hub_(bf16_)?kernelILi(\d+)ELi(\d+)E(?:Li(\d+)E|Lb([01])E)E", m.group(1))
                if t:   # pass, bf16, GROUP, HPQ, rows in flight (source side) or scores from the gathered row (forward, destination side)
                    key = (t.group(1), bool(t.group(2)), int(t.group(3)), int(t.group(4)), int(t.group(5) if t.group(5) else t.group(6)))
                    hub[key] = (int(m.group(2)), int(m.group(3)))
                t = re.search(r"gatmh_rows_(forward|dst|src)_merge_kernelILi(\d+)ELi(\d+)EE", m.group(1))
                if t:
                    merge[(t.group(1), int(t.group(2)), int(t.group(3)))] = (int(m.group(2)), int(m.group(3)))
    return hub, merge


def test_every_hub_instantiation_is_present_and_fits_without_spills():
    hub, merge = _kernels()
    edge = [(g, h, 1) for g, h in FORMS] + [(32, 1, 0), (64, 1, 0)]     # (rows of 96, 160, 192, 224 floats gather their scores)
    one = {("forward",) + f for f in edge} | {("dst",) + f for f in edge} | {("src", g, h, 2 if h == 4 else 4) for g, h in FORMS}
    want = {(k[0], b) + k[1:] for k in one for b in (False, True)}
    assert set(hub) == want, sorted(set(hub) ^ want)
    assert len(hub) == 62
    want_merge = {(p, g, h) for p in ("forward", "dst", "src") for g, h in FORMS}
    assert set(merge) == want_merge, sorted(set(merge) ^ want_merge)
    for name, ks in (("hub", hub), ("merge", merge)):
        for key, (vgpr, spill) in sorted(ks.items()):
            print("gatmh_rows", name, "kernel", key, "vgprs", vgpr, "spilled", spill)
            assert spill == 0, (key, vgpr, spill)
            assert vgpr <= 128, (key, vgpr)
