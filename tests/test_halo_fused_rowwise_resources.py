"""The send forms of dory_halo_fused_pack_rowwise (csrc/elementwise.hip: tanh_backward_send_kernel, tanh_forward_send_kernel,
softmax_rows_send_kernel) in the code objects inside the built library, read as tests/test_halo_exact_resources.py reads the exact
kernels' (no GPU needed): they exist, every instantiation, and use no scratch; the kernels they stand beside are what they were --
registers, LDS, scratch and code size of tanh_backward_kernel, tanh_forward_kernel and the softmax_xent_kernel instantiations equal
the values recorded from a build of the commit before the switch; and the two new entry points are exported and bound."""
import ctypes
import os

import pytest

from test_halo_exact_resources import FIELDS, kernels

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# recorded from a build of the parent commit (b9dbbc4) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory20tanh_backward_kernelEmjPKfjS1_jPfj": (34, 0, 42, 0, 0, 0, 0, 1436),
    "_ZN4dory19tanh_forward_kernelEmjPKfjPfj": (16, 0, 34, 0, 0, 0, 0, 1092),
    "_ZN4dory19softmax_xent_kernelILi8EEEvjjPKfjS2_jPfjfmmi": (22, 0, 24, 0, 0, 0, 0, 1588),
    "_ZN4dory19softmax_xent_kernelILi16EEEvjjPKfjS2_jPfjfmmi": (22, 0, 24, 0, 0, 0, 0, 1648),
    "_ZN4dory19softmax_xent_kernelILi32EEEvjjPKfjS2_jPfjfmmi": (22, 0, 24, 0, 0, 0, 0, 1732),
    "_ZN4dory19softmax_xent_kernelILi64EEEvjjPKfjS2_jPfjfmmi": (22, 0, 24, 0, 0, 0, 0, 1800),
}
# stem -> instantiations: three wire forms of each tanh kernel; four lanes-per-row counts x {fp32, bf16} of the softmax kernel
NEW = {"tanh_backward_send_kernel": 3, "tanh_forward_send_kernel": 3, "softmax_rows_send_kernel": 8}
# the stems the other resource tests count: no new kernel's name may contain one
COUNTED_STEMS = ("gemm_dma_", "splitk_reduce_", "gather_rows_exact_kernel", "scatter_rows_exact_kernel", "gather_rows_bf16_kernel",
                 "scatter_rows_bf16_kernel", "zero_rows_pad_kernel", "permute_rows_kernel", "bf16_rows_kernel")


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_send_kernels_exist_without_scratch(ks):
    for stem, count in NEW.items():
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == count, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(stem, n, rec, "code bytes", v[-1])
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 64, (n, rec)
            assert not any(s in n for s in COUNTED_STEMS), n


def test_parent_kernels_keep_their_resources(ks):
    assert {n for n in ks if "softmax_xent_kernel" in n or "tanh_backward_kernel" in n or "tanh_forward_kernel" in n} == set(PARENT)
    for name, want in PARENT.items():
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)


def test_entry_points_exported_and_bound():
    import dorylus_amd as da
    lib = ctypes.CDLL(da.LIB_PATH)
    for name in ("dory_halo_fused_pack_rowwise", "dory_halo_fused_pack_rowwise_stats"):
        assert hasattr(lib, name), name
    assert callable(da.Context.halo_fused_pack_rowwise) and callable(da.Context.halo_fused_pack_rowwise_stats)
    from dorylus_amd import _lib
    src = open(_lib.__file__).read()
    assert '"dory_halo_fused_pack_rowwise": [vp, i32]' in src and '"dory_halo_fused_pack_rowwise_stats": [vp, C.POINTER(u64), C.POINTER(u64)]' in src
