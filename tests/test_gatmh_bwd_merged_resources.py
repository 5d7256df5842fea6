"""The kernels of dory_gatmh_bwd_merged_exchange (csrc/gat_mh_sweep.hip: gatmh_dst_rowwise_send_kernel; csrc/elementwise.hip:
gather_rows_pair_kernel, scatter_rows_pair_kernel) in the code objects inside the built library, read as
tests/test_halo_exact_resources.py reads the exact kernels' (no GPU needed): they exist, every instantiation, with no scratch, no
spills, no LDS and at most 64 VGPRs (512 VGPRs per SIMD lane / 64 = 8 waves: full occupancy for a streaming kernel); no name
contains a stem another resource test counts; the kernels they stand beside are what they were -- registers, LDS, scratch and code
size of gatmh_dst_rowwise_kernel, gather_rows_kernel, scatter_rows_kernel and zero_rows_pad_kernel equal the values recorded from a
build of the commit before the switch; and the five entry points are exported and bound."""
import ctypes

import pytest

from test_halo_exact_resources import FIELDS, kernels
from test_halo_fused_rowwise_resources import COUNTED_STEMS

# recorded from a build of the parent commit (89d4a5e) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory24gatmh_dst_rowwise_kernelENS_9GatMhArgsEiPKfS2_S2_S2_S2_S2_S2_PfS3_P15HIP_vector_typeIfLj4EEj": (18, 0, 31, 0, 0, 0, 0, 1512),
    "_ZN4dory18gather_rows_kernelEPfPKfjjPKjj": (17, 0, 32, 0, 0, 0, 0, 916),
    "_ZN4dory19scatter_rows_kernelEPfPKfjjPKjj": (20, 0, 32, 0, 0, 0, 0, 920),
    "_ZN4dory20zero_rows_pad_kernelEPfjjjPKjj": (19, 0, 31, 0, 0, 0, 0, 868),
}
# stem -> instantiations (none is a template)
NEW = {"gatmh_dst_rowwise_send_kernel": 1, "gather_rows_pair_kernel": 1, "scatter_rows_pair_kernel": 1}
ENTRY_POINTS = ("dory_gatmh_bwd_merged_exchange", "dory_gatmh_bwd_merged_exchange_stats", "dory_gatmh_bwd_wire_row", "dory_gatmh_bwd_pack",
                "dory_gatmh_bwd_unpack")


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_new_kernels_exist_without_scratch_or_lds(ks):
    for stem, count in NEW.items():
        found = {n: v for n, v in ks.items() if stem in n}
        assert len(found) == count, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(stem, n, rec, "code bytes", v[-1])
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 64, (n, rec)
            assert not any(s in n for s in COUNTED_STEMS), n


def test_no_new_name_is_counted_by_an_older_test(ks):
    """the older files pick their kernels by substring: the parent kernels' own stems must still match exactly one name each"""
    for stem in ("gatmh_dst_rowwise_kernel", "gather_rows_kernel", "scatter_rows_kernel", "zero_rows_pad_kernel"):
        assert len([n for n in ks if stem in n]) == 1, (stem, [n for n in ks if stem in n])


def test_parent_kernels_keep_their_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)


def test_entry_points_exported_and_bound():
    import dorylus_amd as da
    from dorylus_amd import _lib
    lib = ctypes.CDLL(da.LIB_PATH)
    src = open(_lib.__file__).read()
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
        assert name in da.SYMBOLS and '"%s": [vp' % name in src, name
        assert callable(getattr(da.Context, name[len("dory_"):])), name
