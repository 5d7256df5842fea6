"""The register budget of the carry kernels of the multi-head GAT's row-gather family (csrc/gat_mh_rows.hip,
dory_gatmh_row_gather_edge_split), read from the code objects inside the built library as
tests/test_gatmh_row_gather_overlap_resources.py reads the list kernels (no GPU needed).

A carry kernel walks a row as two ranges of the local-first ids -- the local entries and the self edge, then the ghost entries -- and
parks or loads the row's state between them where the launch says so: which ranges it walks is a kernel argument, so the three walks
are one body of machine code.  The condition is the family's: at most 128 vector registers -- four waves per SIMD, what a
latency-bound gather lives on -- no spills, and every instantiation the launchers can select present, in fp32 and narrow bf16: the
forms of the one-pass kernels, for the forward and the source side (the destination-side edge pass has no exchange to hide behind and
no carry form; there is no wide carry form).  The carry kernels stand beside the family's other kernels: every gatmh_rows* kernel of a
build of the parent commit (tests/golden/gatmh_row_gather_edge_split_parent_kernels.txt) is still there with its vector registers."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
FORMS = [(g, 1) for g in (8, 16, 32, 64)] + [(g, 2) for g in (8, 16, 32)] + [(g, 4) for g in (8, 16)]


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: (vector registers, spilled)} of every gatmh_rows* kernel in the library"""
    lib = os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm tools missing")
    found = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True,
                                   text=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", notes):
                if "gatmh_rows" in m.group(1):
                    found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return found


def test_every_carry_instantiation_is_present_and_fits_without_spills(kernels):
    found, names = {}, [n for n in kernels if "_carry_" in n]
    for name in names:
        t = re.search(r"gatmh_rows_(forward|src)_carry_(bf16_)?kernelILi(\d+)ELi(\d+)E(?:Li(\d+)E|Lb([01])E)E", name)
        assert t, name                                       # nothing else is named *_carry_*
        # pass, bf16, GROUP, HPQ, rows in flight (source side) or scores from the gathered row (forward)
        key = (t.group(1), bool(t.group(2)), int(t.group(3)), int(t.group(4)), int(t.group(5) if t.group(5) else t.group(6)))
        found[key] = kernels[name]
    edge = [(g, h, 1) for g, h in FORMS] + [(32, 1, 0), (64, 1, 0)]     # (rows of 96, 160, 192, 224 floats gather their scores)
    one = {("forward",) + f for f in edge} | {("src", g, h, 2 if h == 4 else 4) for g, h in FORMS}
    want = {(k[0], b) + k[1:] for k in one for b in (False, True)}
    assert set(found) == want, sorted(set(found) ^ want)
    assert len(found) == 40 and len(names) == 40, names      # (11 forward + 9 source-side forms; fp32 / bf16)
    for key, (vgpr, spill) in sorted(found.items()):
        print("gatmh_rows carry kernel", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)


def test_the_familys_other_kernels_keep_the_parent_builds_registers(kernels):
    parent = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "gatmh_row_gather_edge_split_parent_kernels.txt")):
        if line.strip() and not line.startswith("#"):
            name, vgpr, spill = line.split()
            parent[name] = (int(vgpr), int(spill))
    assert len(parent) == 273, len(parent)
    old = {n: r for n, r in kernels.items() if "_carry_" not in n}
    assert set(old) == set(parent), sorted(set(old) ^ set(parent))          # no kernel renamed, none added under the counted names
    for name, res in sorted(old.items()):
        assert res == parent[name], (name, res, parent[name])
