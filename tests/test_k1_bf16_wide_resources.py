"""The register budget of K1's wide bf16 kernels (csrc/spmm.hip, dory_k1_bf16_wide: spmm_rows_bf16x8_kernel), read from the code
objects inside the built library as tests/test_gatmh_row_gather_bf16_wide_resources.py reads its family's (no GPU needed).

A wide lane keeps two float4 sums per chunk where a narrow lane keeps one, and 16 bytes of raw bf16 per edge in flight and chunk
where a narrow lane keeps 8.  The condition: at most 128 vector registers -- four waves per SIMD, the floor the fp32 family already
runs at (spmm_rows_kernel<32, 3>) -- and no spills; exactly the instantiations the rule of csrc/k1_shapes.hpp can select are present;
and the 16 narrow / fp32 instantiations and the three long-row kernels, which the wide form runs beside and must not have touched,
keep the vector-register counts of a build of the parent commit (tests/golden/k1_bf16_wide_parent_kernels.txt)."""
import os
import re
import shutil
import subprocess
import tempfile

import pytest

import k1_bf16_wide_ref as kr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
NARROW_FORMS = [(8, 1), (16, 1), (32, 1), (64, 1), (32, 3), (64, 2), (64, 3), (64, 4)]


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: (vector registers, spilled)} of every spmm_rows / spmm_longrow kernel in the library"""
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
                if "spmm_rows" in m.group(1) or "spmm_longrow" in m.group(1):
                    found[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return found


def test_exactly_the_instantiations_of_the_rule_are_present_and_fit_without_spills(kernels):
    wide = {}
    for name, res in kernels.items():
        if "bf16x8" in name:
            t = re.search(r"spmm_rows_bf16x8_kernelILi(\d+)ELi(\d+)EE", name)
            assert t, name                                   # nothing else is named *bf16x8* among K1's kernels
            wide[(int(t.group(1)), int(t.group(2)))] = res
    assert sorted(wide) == kr.WIDE_FORMS, sorted(wide)
    assert len([n for n in kernels if "bf16x8" in n]) == len(kr.WIDE_FORMS)
    for key, (vgpr, spill) in sorted(wide.items()):
        print("spmm_rows_bf16x8_kernel", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0, (key, vgpr, spill)
        assert vgpr <= 128, (key, vgpr)


def test_the_narrow_fp32_and_long_row_kernels_keep_the_parent_builds_registers(kernels):
    parent = {}
    for line in open(os.path.join(ROOT, "tests", "golden", "k1_bf16_wide_parent_kernels.txt")):
        if line.strip() and not line.startswith("#"):
            name, vgpr = line.split()
            parent[name] = int(vgpr)
    want = {f"spmm_rows{bf}_kernelILi{g}ELi{c}EE" for bf in ("", "_bf16") for g, c in NARROW_FORMS}
    want |= {"spmm_longrow_kernelE", "spmm_longrow_bf16_kernelE", "spmm_longrow_reduce_kernelE"}
    assert len(parent) == 19 and all(any(w in n for n in parent) for w in want), sorted(parent)
    old = {n: r for n, r in kernels.items() if "bf16x8" not in n}
    assert set(old) == set(parent), sorted(set(old) ^ set(parent))          # no kernel renamed, none added under the counted names
    for name, (vgpr, spill) in sorted(old.items()):
        assert spill == 0 and vgpr == parent[name], (name, vgpr, spill, parent[name])
