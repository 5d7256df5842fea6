"""The register budget of the list kernels of the multi-head GAT's row-gather family (csrc/gat_mh_rows.hip,
dory_gatmh_row_gather_overlap), read from the code objects inside the built library as tests/test_gatmh_row_gather_hubs_resources.py reads
the hub kernels (no GPU needed).

A pass that runs its interior rows beside the exchange launches a list form twice -- the interior rows, then the other rows: the
one-pass body with its row units named by a list (*_list_kernel), or, where the chunk plan has chunks, the hub body likewise
(*_list_hub_kernel: the hub rows' chunk units first).  The condition is the family's: at most 128 vector registers -- four waves per
SIMD, what a latency-bound gather lives on -- no spills, and every instantiation the launchers can select present, in fp32 and bf16:
the forms of the one-pass kernels, for the forward and the source side (the destination-side edge pass has no exchange to hide behind
and no list form)."""
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
                if "gatmh_rows_" in m.group(1) and "_list_" in m.group(1):
                    names.append(m.group(1))
                t = re.search(r"gatmh_rows_(forward|dst|src)_list_(hub_)?(bf16_)?kernelILi(\d+)ELi(\d+)E(?:Li(\d+)E|Lb([01])E)E", m.group(1))
                if t:   # pass, hub form, bf16, GROUP, HPQ, rows in flight (source side) or scores from the gathered row (forward)
                    key = (t.group(1), bool(t.group(2)), bool(t.group(3)), int(t.group(4)), int(t.group(5)),
                           int(t.group(6) if t.group(6) else t.group(7)))
                    found[key] = (int(m.group(2)), int(m.group(3)))
    return found, names


def test_every_list_instantiation_is_present_and_fits_without_spills():
    found, names = _kernels()
    edge = [(g, h, 1) for g, h in FORMS] + [(32, 1, 0), (64, 1, 0)]     # (rows of 96, 160, 192, 224 floats gather their scores)
    one = {("forward",) + f for f in edge} | {("src", g, h, 2 if h == 4 else 4) for g, h in FORMS}
    want = {(k[0], h, b) + k[1:] for k in one for h in (False, True) for b in (False, True)}
    assert set(found) == want, sorted(set(found) ^ want)
    assert len(found) == 80 and len(names) == 80, names    # (11 forward + 9 source-side forms; one-pass / hub; fp32 / bf16; nothing else named *_list_*)
    for key, (vgpr, spill) in sorted(found.items()):
        print("gatmh_rows list kernel", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)
