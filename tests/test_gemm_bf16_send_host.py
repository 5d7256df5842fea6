"""dory_gemm_bf16_send without a GPU: the entry points are declared and exported; the sixteen send kernels of csrc/gemm_bf16.hip and
csrc/gemm_bf16_split.hip (send / send16 x NN / NT x both tile widths), read from the code objects inside the built library as
tests/test_gemm_bf16_split_host.py reads K2c's, spill nothing and K2c's stay inside what their LDS footprint allows; and the twelve plain
K2b / K2c kernels keep the vector-register counts of a build of the parent commit (tests/golden/gemm_bf16_send_parent_kernels.txt)."""
import ctypes
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gatmh_row_gather_bf16_wide_rate import kernel_notes
    lib = os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    return kernel_notes(lib)


def test_symbols_are_declared_and_exported():
    import dorylus_amd
    header = open(os.path.join(ROOT, "include", "dorylus_hip.h")).read()
    lib = ctypes.CDLL(dorylus_amd.LIB_PATH)
    for s in ("dory_gemm_bf16_send", "dory_gemm_bf16_send_stats"):
        assert re.search(r"\bint %s\(dory_ctx \*ctx" % s, header) and s in dorylus_amd.SYMBOLS and hasattr(lib, s), s


def test_the_sixteen_send_kernels_fit_without_spills(kernels):
    found = {}
    for name, res in kernels.items():
        t = re.search(r"gemm_bf16(x3)?_send(16)?_kernelILi(\d+)E(?:Li\d+E){4}Lb0ELb([01])ELi32EE", name)
        if t:
            found[("K2c" if t.group(1) else "K2b", "bf16" if t.group(2) else "fp32", int(t.group(3)), "NT" if t.group(4) == "0" else "NN")] = res
    assert sorted(found) == sorted((k, w, bn, f) for k in ("K2b", "K2c") for w in ("bf16", "fp32") for bn in (64, 128) for f in ("NN", "NT")), sorted(found)
    for (k, w, bn, f), (vgpr, spill) in sorted(found.items()):
        print(k, "send kernel,", w, "wire", bn, f, "vgprs", vgpr, "spilled", spill)
        # K2c: LDS holds three workgroups per CU at BN = 64 and two at 128 -- the registers must not lower that
        assert spill == 0 and (k == "K2b" or vgpr <= (168 if bn == 64 else 256)), (k, w, bn, f, vgpr, spill)


def test_the_plain_kernels_keep_the_parents_registers(kernels):
    parent = dict(line.split() for line in open(os.path.join(ROOT, "tests", "golden", "gemm_bf16_send_parent_kernels.txt"))
                  if line.strip() and not line.startswith("#"))
    plain = {n: r for n, r in kernels.items() if re.search(r"gemm_bf16(x3)?_kernel", n)}
    assert len(parent) == 12 and set(plain) == set(parent), sorted(set(plain) ^ set(parent))
    for name, (vgpr, spill) in plain.items():
        assert spill == 0 and vgpr == int(parent[name]), (name, vgpr, spill, parent[name])
