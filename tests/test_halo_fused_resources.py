"""The kernels of the fused halo pack (csrc/gemm.hip: gemm_dma_send_kernel, gemm_dma_send_kernel_occ4, splitk_reduce_send_kernel)
in the code objects inside the built library, read as tests/test_halo_exact_resources.py reads its own (no GPU needed): the five
exist, none has scratch or spills, the 128-wide ones stay within the 128 VGPRs of amdgpu_waves_per_eu(4, 4); and the GEMM kernels
that were there before keep what a build of the commit before the feature gave them -- registers, LDS, scratch and code size."""
import pytest

from test_halo_exact_resources import FIELDS, kernels

# recorded from a build of the parent commit (779fd03) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory20splitk_reduce_kernelEPfPKfjjjjS0_j": (40, 0, 67, 0, 0, 0, 0, 1568),
    "_ZN4dory20gemm_dma_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb0ELb1ELi16EEEvNS_8GemmArgsEjPf": (117, 0, 52, 0, 0, 32768, 0, 16724),
    "_ZN4dory20gemm_dma_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb0ELb0ELi16EEEvNS_8GemmArgsEjPf": (115, 0, 52, 0, 0, 32768, 0, 16632),
    "_ZN4dory20gemm_dma_kernel_occ4ILi128ELi2ELi2ELi2ELi2ELb1ELb1ELi16EEEvNS_8GemmArgsEjPf": (113, 0, 52, 0, 0, 32768, 0, 16688),
    "_ZN4dory15gemm_dma_kernelILi64ELi4ELi1ELi1ELi2ELb0ELb1ELi16EEEvNS_8GemmArgsEjPf": (76, 32, 50, 0, 0, 24576, 0, 9496),
    "_ZN4dory15gemm_dma_kernelILi64ELi4ELi1ELi1ELi2ELb0ELb0ELi16EEEvNS_8GemmArgsEjPf": (76, 32, 50, 0, 0, 24576, 0, 9404),
    "_ZN4dory15gemm_dma_kernelILi64ELi4ELi1ELi1ELi2ELb1ELb1ELi16EEEvNS_8GemmArgsEjPf": (76, 32, 50, 0, 0, 24576, 0, 9444),
}
# stem -> (instantiations, VGPR bound): NN and NT of each tile shape, one reduce kernel
NEW = {"gemm_dma_send_kernel_occ4I": (2, 128), "gemm_dma_send_kernelI": (2, 128), "splitk_reduce_send_kernel": (1, 64)}


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_send_kernels_exist_without_scratch(ks):
    for stem, (count, vgprs) in NEW.items():
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == count, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(n, rec, "code bytes", v[-1])
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["vgpr_count"] <= vgprs, (n, rec)
    # NN (B k-major) and NT (B row-major) of the 128-wide tile, no TN
    wide = sorted(n for n in ks if "gemm_dma_send_kernel_occ4I" in n)
    assert ["Lb0ELb0E" in n or "Lb0ELb1E" in n for n in wide] == [True, True], wide


def test_existing_gemm_kernels_keep_the_parents_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)
