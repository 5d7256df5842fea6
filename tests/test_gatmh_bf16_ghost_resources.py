"""The kernels of dory_gatmh_bf16_ghosts (csrc/gat_mh.hip: gatmh_scores4_bf16_kernel, gatmh_scores_bf16_kernel; csrc/elementwise.hip:
scatter_rows_pair_bf16_keep_kernel) in the code objects inside the built library, read as tests/test_halo_bf16_ghost_resources.py reads
its own (no GPU needed): each exists once, without scratch, spills or LDS, its registers are recorded; the siblings they stand beside
keep what a build of the commit before the feature gave them -- registers, LDS, scratch and code size --, and every kernel that build
had (tests/golden/gatmh_bf16_ghosts_parent_kernels.txt: the mangled names) is still there under its name."""
import os

import pytest

from test_halo_exact_resources import FIELDS, ROOT, kernels

# recorded from a build of the parent commit (c30fced) with the same compiler: FIELDS in order, then the code size in bytes
PARENT = {
    "_ZN4dory19gatmh_scores_kernelEjjjPKfjS1_S1_PfS2_j": (20, 0, 24, 0, 0, 0, 0, 1012),
    "_ZN4dory20gatmh_scores4_kernelEjjjjPKfjS1_S1_PfS2_j": (16, 0, 26, 0, 0, 0, 0, 1480),
    "_ZN4dory24scatter_rows_pair_kernelEPfjjS0_jjPK15HIP_vector_typeIfLj4EEPKjj": (24, 0, 33, 0, 0, 0, 0, 1016),
    "_ZN4dory29scatter_rows_pair_bf16_kernelEPfjjS0_jjPK15HIP_vector_typeIjLj4EEPKjj": (18, 0, 34, 0, 0, 0, 0, 616),
}
# the new kernels as this commit's build gives them (vgpr_count, sgpr_count): recorded, not a bound -- the bound is "no more than 64"
NEW = {"gatmh_scores4_bf16_kernel": (14, 26), "gatmh_scores_bf16_kernel": (18, 24), "scatter_rows_pair_bf16_keep_kernel": (22, 27)}


@pytest.fixture(scope="module")
def ks():
    return kernels()


def test_new_kernels_exist_once_without_scratch_spills_or_lds(ks):
    for stem, recorded in NEW.items():
        found = {n: v for n, v in ks.items() if "4dory%d%sE" % (len(stem), stem) in n}
        assert len(found) == 1, (stem, sorted(found))
        for n, v in found.items():
            rec = dict(zip(FIELDS, v))
            print(n, rec, "code bytes", v[-1], "recorded (vgpr, sgpr):", recorded)
            assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
            assert rec["group_segment_fixed_size"] == 0 and rec["vgpr_count"] <= 64 and rec["agpr_count"] == 0, (n, rec)


def test_siblings_keep_the_parents_resources(ks):
    for name, want in PARENT.items():
        assert name in ks, name
        print(name, ks[name])
        assert ks[name] == want, (name, dict(zip(FIELDS + ("code_bytes",), ks[name])), "parent:", want)


def test_every_kernel_of_the_parent_keeps_its_name(ks):
    names = open(os.path.join(ROOT, "tests", "golden", "gatmh_bf16_ghosts_parent_kernels.txt")).read().split()
    assert len(names) > 500
    gone = [n for n in names if n not in ks]
    assert not gone, gone
