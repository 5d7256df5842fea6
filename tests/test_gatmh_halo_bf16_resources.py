"""The kernels of dory_gatmh_halo_bf16 (csrc/elementwise.hip: gather_rows_pair_bf16_kernel, scatter_rows_pair_bf16_kernel;
csrc/gat_mh_sweep.hip: gatmh_dst_rowwise_send_bf16_kernel) in the code objects inside the built library, read as
tests/test_gatmh_bwd_merged_resources.py reads its kernels' (no GPU needed): they exist, one instantiation each, with no scratch, no
spills, no LDS and at most 64 VGPRs; no name contains a stem another resource test counts; the kernels they stand beside are what
they were -- registers, LDS, scratch and code size of the fp32 pair kernels, the two row-wise kernels and the bf16 row kernels equal
the values recorded from a build of the commit before the switch; and the three entry points are exported and bound."""
import ctypes

import pytest

from test_halo_exact_resources import FIELDS, kernels
from test_halo_fused_rowwise_resources import COUNTED_STEMS

# recorded from a build of the parent commit (a0f0671) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory23gather_rows_pair_kernelEP15HIP_vector_typeIfLj4EEPKfjjS4_jjPKjj": (17, 0, 36, 0, 0, 0, 0, 972),
    "_ZN4dory24scatter_rows_pair_kernelEPfjjS0_jjPK15HIP_vector_typeIfLj4EEPKjj": (24, 0, 33, 0, 0, 0, 0, 1016),
    "_ZN4dory24gatmh_dst_rowwise_kernelENS_9GatMhArgsEiPKfS2_S2_S2_S2_S2_S2_PfS3_P15HIP_vector_typeIfLj4EEj": (18, 0, 31, 0, 0, 0, 0, 1512),
    "_ZN4dory29gatmh_dst_rowwise_send_kernelENS_9GatMhArgsEiPKfS2_S2_S2_S2_S2_S2_PfS3_P15HIP_vector_typeIfLj4EEjNS_9GatmhSendE":
        (24, 0, 36, 0, 0, 0, 0, 1900),
    "_ZN4dory23gather_rows_bf16_kernelILb0EEEvP15HIP_vector_typeIjLj2EEPKfjjjPKjj": (17, 0, 33, 0, 0, 0, 0, 1048),
    "_ZN4dory23gather_rows_bf16_kernelILb1EEEvP15HIP_vector_typeIjLj2EEPKfjjjPKjj": (18, 0, 34, 0, 0, 0, 0, 1032),
    "_ZN4dory24scatter_rows_bf16_kernelILb0EEEvPfPK15HIP_vector_typeIjLj2EEjjPKjj": (16, 0, 34, 0, 0, 0, 0, 1104),
    "_ZN4dory24scatter_rows_bf16_kernelILb1EEEvPfPK15HIP_vector_typeIjLj2EEjjPKjj": (16, 0, 34, 0, 0, 0, 0, 976),
    "_ZN4dory29scatter_rows_bf16_keep_kernelILi4EEEvPtPK15HIP_vector_typeIjLj2EEjjPKjj": (15, 0, 34, 0, 0, 0, 0, 936),
}
# stem -> instantiations (none is a template)
NEW = {"gather_rows_pair_bf16_kernel": 1, "scatter_rows_pair_bf16_kernel": 1, "gatmh_dst_rowwise_send_bf16_kernel": 1}
ENTRY_POINTS = ("dory_gatmh_halo_bf16", "dory_gatmh_halo_bf16_stats", "dory_gatmh_bwd_wire_do")


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
    """the older files pick their kernels by substring: the siblings' own stems must still match as many names as before"""
    for stem, count in (("gather_rows_pair_kernel", 1), ("scatter_rows_pair_kernel", 1), ("gatmh_dst_rowwise_kernel", 1),
                        ("gatmh_dst_rowwise_send_kernel", 1), ("gather_rows_bf16_kernel", 2), ("scatter_rows_bf16_kernel", 2),
                        ("scatter_rows_bf16_keep_kernel", 1)):
        assert len([n for n in ks if stem in n]) == count, (stem, [n for n in ks if stem in n])


def test_sibling_kernels_keep_their_resources(ks):
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
