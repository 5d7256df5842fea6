"""The kernels of dory_halo_bf16_ghosts (csrc/elementwise.hip: scatter_rows_bf16_keep_kernel, widen_rows_bf16_kernel) in the code
objects inside the built library, read as tests/test_halo_exact_resources.py reads its own (no GPU needed): both exist, one
instantiation each, without scratch, spills or LDS; and bf16_rows_kernel, the four instantiations of the bf16 pack and unpack and the
six older K6 kernels keep what a build of the commit before the feature gave them -- registers, LDS, scratch and code size."""
import pytest

from test_halo_exact_resources import FIELDS, kernels

# recorded from a build of the parent commit (bf72d56) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory16bf16_rows_kernelEPK15HIP_vector_typeIfLj4EEPS0_IjLj2EEm": (10, 0, 18, 0, 0, 0, 0, 232),
    "_ZN4dory23gather_rows_bf16_kernelILb0EEEvP15HIP_vector_typeIjLj2EEPKfjjjPKjj": (17, 0, 33, 0, 0, 0, 0, 1048),
    "_ZN4dory23gather_rows_bf16_kernelILb1EEEvP15HIP_vector_typeIjLj2EEPKfjjjPKjj": (18, 0, 34, 0, 0, 0, 0, 1032),
    "_ZN4dory24scatter_rows_bf16_kernelILb0EEEvPfPK15HIP_vector_typeIjLj2EEjjPKjj": (16, 0, 34, 0, 0, 0, 0, 1104),
    "_ZN4dory24scatter_rows_bf16_kernelILb1EEEvPfPK15HIP_vector_typeIjLj2EEjjPKjj": (16, 0, 34, 0, 0, 0, 0, 976),
    "_ZN4dory18gather_rows_kernelEPfPKfjjPKjj": (17, 0, 32, 0, 0, 0, 0, 916),
    "_ZN4dory19scatter_rows_kernelEPfPKfjjPKjj": (20, 0, 32, 0, 0, 0, 0, 920),
    "_ZN4dory20zero_rows_pad_kernelEPfjjjPKjj": (19, 0, 31, 0, 0, 0, 0, 868),
    "_ZN4dory24gather_rows_exact_kernelEPfPKfjjPKjjj": (18, 0, 31, 0, 0, 0, 0, 1000),
    "_ZN4dory25scatter_rows_exact_kernelEPfPKfjjPKjjj": (20, 0, 31, 0, 0, 0, 0, 1740),
    "_ZN4dory19permute_rows_kernelEPfPKfjPKjji": (15, 0, 33, 0, 0, 0, 0, 896),
}
NEW = ("scatter_rows_bf16_keep_kernel", "widen_rows_bf16_kernel")


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_ghost_twin_kernels_exist_without_scratch_spills_or_lds(ks):
    for stem in NEW:
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == 1, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(n, rec, "code bytes", v[-1])
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 64 and rec["agpr_count"] == 0, (n, rec)


def test_existing_bf16_and_k6_kernels_keep_the_parents_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)
