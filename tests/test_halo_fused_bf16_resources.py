"""The kernels of the fused halo pack's bf16 form (csrc/gemm.hip: gemm_dma_send16_kernel, gemm_dma_send16_kernel_occ4,
splitk_reduce_send16_kernel) in the code objects inside the built library, read as tests/test_halo_exact_resources.py reads its own
(no GPU needed): NN and NT of both tile shapes and one reduce form exist, none has scratch or spills, the 128-wide ones stay within
the 128 VGPRs of amdgpu_waves_per_eu(4, 4); every GEMM kernel that was there before -- the three fp32 send kernels among them --
keeps what a build of the commit before the feature gave it: registers, LDS, scratch and code size; and the switch is there, in the
library and on Context."""
import ctypes

import pytest

from test_halo_exact_resources import FIELDS, kernels

# recorded from a build of the parent commit (fe4d5f5) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory15gemm_dma_kernelILi64ELi4ELi1ELi1ELi2ELb0ELb0ELi16EEEvNS_8GemmArgsEjPf": (76, 32, 50, 0, 0, 24576, 0, 9404),
    "_ZN4dory15gemm_dma_kernelILi64ELi4ELi1ELi1ELi2ELb0ELb1ELi16EEEvNS_8GemmArgsEjPf": (76, 32, 50, 0, 0, 24576, 0, 9496),
    "_ZN4dory15gemm_dma_kernelILi64ELi4ELi1ELi1ELi2ELb1ELb1ELi16EEEvNS_8GemmArgsEjPf": (76, 32, 50, 0, 0, 24576, 0, 9444),
    "_ZN4dory20gemm_dma_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb0ELb0ELi16EEEvNS_8GemmArgsEjPf": (115, 0, 52, 0, 0, 32768, 0, 16632),
    "_ZN4dory20gemm_dma_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb0ELb1ELi16EEEvNS_8GemmArgsEjPf": (117, 0, 52, 0, 0, 32768, 0, 16724),
    "_ZN4dory20gemm_dma_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb1ELb1ELi16EEEvNS_8GemmArgsEjPf": (113, 0, 52, 0, 0, 32768, 0, 16688),
    "_ZN4dory20gemm_dma_send_kernelILi64ELi4ELi1ELi1ELi2ELb0ELb0ELi16EEEvNS_8GemmArgsEjPfNS_8GemmSendE": (92, 32, 60, 0, 0, 24576, 0, 13492),
    "_ZN4dory20gemm_dma_send_kernelILi64ELi4ELi1ELi1ELi2ELb0ELb1ELi16EEEvNS_8GemmArgsEjPfNS_8GemmSendE": (92, 32, 60, 0, 0, 24576, 0, 13600),
    "_ZN4dory20splitk_reduce_kernelEPfPKfjjjjS0_j": (40, 0, 67, 0, 0, 0, 0, 1568),
    "_ZN4dory25gemm_dma_send_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb0ELb0ELi16EEEvNS_8GemmArgsEjPfNS_8GemmSendE": (115, 0, 94, 0, 0, 32768, 0, 23980),
    "_ZN4dory25gemm_dma_send_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb0ELb1ELi16EEEvNS_8GemmArgsEjPfNS_8GemmSendE": (117, 0, 94, 0, 0, 32768, 0, 24072),
    "_ZN4dory25splitk_reduce_send_kernelEPfPKfjjjjS0_jNS_8GemmSendE": (39, 0, 77, 0, 0, 0, 0, 2216),
}
# stem -> (instantiations, VGPR bound): NN and NT of each tile shape, one reduce kernel
NEW = {"gemm_dma_send16_kernel_occ4I": (2, 128), "gemm_dma_send16_kernelI": (2, 128), "splitk_reduce_send16_kernel": (1, 64)}
# what tests/test_halo_fused_resources.py counts the fp32 send kernels by: no new name may contain one
OLD_STEMS = ("gemm_dma_send_kernelI", "gemm_dma_send_kernel_occ4I", "splitk_reduce_send_kernel")


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_send16_kernels_exist_without_scratch(ks):
    for stem, (count, vgprs) in NEW.items():
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == count, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(n, rec, "code bytes", v[-1])
            assert not any(old in n for old in OLD_STEMS), n
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["vgpr_count"] <= vgprs, (n, rec)
    # NN (B k-major) and NT (B row-major) of each tile shape, no TN
    for stem in ("gemm_dma_send16_kernel_occ4I", "gemm_dma_send16_kernelI"):
        forms = sorted(n for n in ks if stem in n)
        assert ["Lb0ELb0E" in n or "Lb0ELb1E" in n for n in forms] == [True, True], forms
        assert len({("Lb0ELb0E" in n) for n in forms}) == 2, forms


def test_every_gemm_kernel_of_the_parent_keeps_its_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)
    # and nothing else in the GEMM family but the new kernels
    family = {n for n in ks if "gemm_dma_" in n or "splitk_reduce_" in n}
    extra = family - set(PARENT)
    assert all(any(stem in n for stem in NEW) for n in extra) and len(extra) == sum(c for c, _ in NEW.values()), sorted(extra)


def test_switch_is_exported_and_bound():
    import dorylus_amd as da
    lib = ctypes.CDLL(da.LIB_PATH)
    assert hasattr(lib, "dory_halo_fused_pack_bf16") and hasattr(lib, "dory_halo_fused_pack_bf16_stats")
    assert callable(getattr(da.Context, "halo_fused_pack_bf16", None)) and callable(getattr(da.Context, "halo_fused_pack_bf16_stats", None))
    for name in ("dory_halo_fused_pack_bf16", "dory_halo_fused_pack_bf16_stats"):
        assert getattr(da.load(), name).argtypes is not None, name
