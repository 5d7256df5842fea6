"""dory_gemm_bf16 without a GPU: the entry points are declared and exported, and the six kernels of csrc/gemm_bf16.hip (NN / NT / TN at
both tile widths), read from the code objects inside the built library as tests/test_k1_bf16_wide_resources.py reads K1's, spill
nothing; the 128-wide TN form keeps the four waves per SIMD of K2's 128 x 128 form (at most 128 vector registers), and K2's own
kernels keep the vector-register counts of a build of the parent commit (tests/golden/gemm_bf16_parent_kernels.txt)."""
import ctypes
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels():
    """{kernel name: (vector registers, spilled)} of the gfx950 code objects inside the library"""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gatmh_row_gather_bf16_wide_rate import kernel_notes
    lib = os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    return kernel_notes(lib)


def test_symbols_are_declared_and_exported():
    import dorylus_amd
    header = open(os.path.join(ROOT, "include", "dorylus_hip.h")).read()
    lib = ctypes.CDLL(dorylus_amd.LIB_PATH)
    for s in ("dory_gemm_bf16", "dory_gemm_bf16_stats"):
        assert re.search(r"\bint %s\(dory_ctx \*ctx" % s, header) and s in dorylus_amd.SYMBOLS and hasattr(lib, s), s


def test_the_kernels_fit_without_spills_and_k2_keeps_its_registers(kernels):
    new = {}
    for name, res in kernels.items():
        t = re.search(r"gemm_bf16_kernel(_occ4)?ILi(\d+)E(?:Li\d+E){4}Lb([01])ELb([01])ELi32EE", name)
        if t:
            new[(int(t.group(2)), t.group(3) + t.group(4), bool(t.group(1)))] = res
    forms = {"01": "NN", "00": "NT", "11": "TN"}
    assert sorted((bn, forms[f]) for bn, f, _ in new) == sorted((bn, f) for bn in (64, 128) for f in forms.values()), sorted(new)
    for (bn, f, occ4), (vgpr, spill) in sorted(new.items()):
        print("gemm_bf16_kernel", bn, forms[f], "occ4" if occ4 else "", "vgprs", vgpr, "spilled", spill)
        assert spill == 0 and (vgpr <= 128 or not occ4) and occ4 == (bn == 128 and f == "11"), (bn, f, occ4, vgpr, spill)
    parent = dict(line.split() for line in open(os.path.join(ROOT, "tests", "golden", "gemm_bf16_parent_kernels.txt"))
                  if line.strip() and not line.startswith("#"))
    k2 = {n: r for n, r in kernels.items() if "gemm_dma" in n or "splitk_reduce" in n}
    assert len(parent) == 17 and set(k2) == set(parent), sorted(set(k2) ^ set(parent))
    for name, (vgpr, spill) in k2.items():
        assert spill == 0 and vgpr == int(parent[name]), (name, vgpr, spill, parent[name])
