"""The kernels of dory_halo_bf16_rows (csrc/elementwise.hip: gather_rows_bf16_kernel, scatter_rows_bf16_kernel, each for tensors whose
ld is a multiple of 4 and for one-column tensors) in the code objects inside the built library, read as
tests/test_halo_exact_resources.py reads its own (no GPU needed): the four exist, none has scratch, spills or LDS; and the K6 kernels
and the bf16 conversion that were there before keep what a build of the commit before the feature gave them -- registers, LDS, scratch
and code size."""
import pytest

from test_halo_exact_resources import FIELDS, kernels

# recorded from a build of the parent commit (895543f) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory16bf16_rows_kernelEPK15HIP_vector_typeIfLj4EEPS0_IjLj2EEm": (10, 0, 18, 0, 0, 0, 0, 232),
    "_ZN4dory18gather_rows_kernelEPfPKfjjPKjj": (17, 0, 32, 0, 0, 0, 0, 916),
    "_ZN4dory19scatter_rows_kernelEPfPKfjjPKjj": (20, 0, 32, 0, 0, 0, 0, 920),
    "_ZN4dory20zero_rows_pad_kernelEPfjjjPKjj": (19, 0, 31, 0, 0, 0, 0, 868),
    "_ZN4dory24gather_rows_exact_kernelEPfPKfjjPKjjj": (18, 0, 31, 0, 0, 0, 0, 1000),
    "_ZN4dory25scatter_rows_exact_kernelEPfPKfjjPKjjj": (20, 0, 31, 0, 0, 0, 0, 1740),
}
# stem -> instantiations (VEC = true / false)
NEW = {"gather_rows_bf16_kernel": 2, "scatter_rows_bf16_kernel": 2}


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_bf16_row_kernels_exist_without_scratch(ks):
    for stem, count in NEW.items():
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == count, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(n, rec, "code bytes", v[-1])
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 64, (n, rec)


def test_existing_k6_kernels_keep_the_parents_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)
