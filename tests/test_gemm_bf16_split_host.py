"""dory_gemm_bf16_split without a GPU: the entry points are declared and exported, and the six kernels of csrc/gemm_bf16_split.hip (NN / NT /
TN at both tile widths), read from the code objects inside the built library as tests/test_gemm_bf16_host.py reads K2b's, spill nothing."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_are_declared_and_exported():
    import dorylus_amd
    header = open(os.path.join(ROOT, "include", "dorylus_hip.h")).read()
    lib = ctypes.CDLL(dorylus_amd.LIB_PATH)
    for s in ("dory_gemm_bf16_split", "dory_gemm_bf16_split_stats"):
        assert re.search(r"\bint %s\(dory_ctx \*ctx" % s, header) and s in dorylus_amd.SYMBOLS and hasattr(lib, s), s


def test_the_six_kernels_fit_without_spills():
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    from gatmh_row_gather_bf16_wide_rate import kernel_notes
    lib = os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so")
    assert os.path.exists(lib), "the library is not built"
    forms = {"01": "NN", "00": "NT", "11": "TN"}
    found = {}
    for name, res in kernel_notes(lib).items():
        t = re.search(r"gemm_bf16x3_kernelILi(\d+)E(?:Li\d+E){4}Lb([01])ELb([01])ELi32EE", name)
        if t:
            found[(int(t.group(1)), forms[t.group(2) + t.group(3)])] = res
    assert sorted(found) == sorted((bn, f) for bn in (64, 128) for f in forms.values()), sorted(found)
    for (bn, f), (vgpr, spill) in sorted(found.items()):
        print("gemm_bf16x3_kernel", bn, f, "vgprs", vgpr, "spilled", spill)
        # LDS holds three workgroups per CU at BN = 64 and two at 128: the registers must not lower that
        assert spill == 0 and vgpr <= (168 if bn == 64 else 256), (bn, f, vgpr, spill)
