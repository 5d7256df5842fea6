"""Option halo_direct_recv adds one kernel (csrc/elementwise.hip: permute_rows_kernel, the row permutation behind uploads and
downloads of wire-ordered ghost tensors) and changes none: read from the code objects inside the built library as
tests/test_halo_exact_resources.py reads them (no GPU needed).  The pack / unpack kernels and the K1s instantiation recorded
there keep the parent's registers, LDS, scratch and code size."""
import pytest

from test_halo_exact_resources import FIELDS, PARENT, kernels


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_permute_kernel_exists_without_scratch(ks):
    found = {n: v for n, v in ks.items() if "permute_rows_kernel" in n}
    assert len(found) == 1, sorted(found)
    for n, v in found.items():
        rec = dict(zip(FIELDS, v))
        print(n, rec, "code bytes", v[-1])
        assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
        assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 32, (n, rec)


def test_pack_and_unpack_kernels_are_the_parents(ks):
    for name, want in PARENT.items():
        assert ks.get(name) == want, (name, ks.get(name), "parent:", want)
    for stem in ("gather_rows_exact_kernel", "scatter_rows_exact_kernel", "zero_rows_pad_kernel"):
        assert sum(stem in n for n in ks) == 1, stem
