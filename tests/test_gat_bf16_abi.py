"""dory_gat_bf16_gather / dory_gat_bf16_gather_stats (include/dorylus_hip.h): the bf16 row gathers of the GAT prototype's
aggregations have entry points of their own beside the option table.  No GPU: the symbols are exported by the built library,
declared in the header with the documented signatures, and bound by dorylus_amd/_lib.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dory_gat_bf16_gather", "dory_gat_bf16_gather_stats")


def _header():
    return open(os.path.join(ROOT, "include", "dorylus_hip.h")).read()


def test_symbols_are_exported():
    lib = ctypes.CDLL(os.path.join(ROOT, "dorylus_amd", "libdorylus_hip.so"))
    for n in NAMES:
        assert hasattr(lib, n), n


def test_header_declares_them():
    h = re.sub(r"\s+", " ", _header())
    assert "int dory_gat_bf16_gather(dory_ctx *ctx, int mode, int wide);" in h
    assert ("int dory_gat_bf16_gather_stats(dory_ctx *ctx, uint64_t *k1s, uint64_t *k1s_wide, uint64_t *k1, "
            "uint64_t *fp32_fallbacks);") in h


def test_lib_binds_them():
    import dorylus_amd._lib as L
    for n in NAMES:
        assert n in L.SYMBOLS, n
    lib = L.load()
    assert [a.__name__ for a in lib.dory_gat_bf16_gather.argtypes] == ["c_void_p", "c_int", "c_int"]
    assert len(lib.dory_gat_bf16_gather_stats.argtypes) == 5
    assert lib.dory_gat_bf16_gather.restype is ctypes.c_int and lib.dory_gat_bf16_gather_stats.restype is ctypes.c_int
    assert callable(L.Context.gat_bf16_gather) and callable(L.Context.gat_bf16_gather_stats)
