"""dory_gemm_bf16_resident without a GPU: the kernels of csrc/gemm_bf16_resident.hip (NN / TN at
both tile widths and the conversion), read from the code objects inside the built library as tests/test_gemm_bf16_host.py reads
K2b's, spill nothing, and the 128-wide forms fit four waves per SIMD; K2b's and K2c's kernels keep the vector-register counts their
file headers record (the counts of a build of the parent commit)."""
import re

from test_gemm_bf16_host import kernels  # noqa: F401  (the fixture)

K2B_K2C = {("bf16", 64, "01"): 92, ("bf16", 64, "00"): 92, ("bf16", 64, "11"): 84, ("bf16", 128, "01"): 140, ("bf16", 128, "00"): 140,
           ("bf16", 128, "11"): 124, ("bf16x3", 64, "01"): 100, ("bf16x3", 64, "00"): 98, ("bf16x3", 64, "11"): 93,
           ("bf16x3", 128, "01"): 144, ("bf16x3", 128, "00"): 142, ("bf16x3", 128, "11"): 134}


def test_the_kernels_fit_without_spills_and_k2b_k2c_keep_their_registers(kernels):
    new, old = {}, {}
    for name, (vgpr, spill) in kernels.items():
        t = re.search(r"gemm_bf16_resident_kernel(_occ4)?ILi(\d+)E(?:Li\d+E){4}Lb([01])ELi32EE", name)
        if t:
            new[(int(t.group(2)), "TN" if t.group(3) == "1" else "NN", bool(t.group(1)))] = (vgpr, spill)
        t = re.search(r"gemm_(bf16|bf16x3)_kernel(?:_occ4)?ILi(\d+)E(?:Li\d+E){4}Lb([01])ELb([01])ELi32EE", name)
        if t:
            old[(t.group(1), int(t.group(2)), t.group(3) + t.group(4))] = (vgpr, spill)
        if "gemm_resident_rows_kernel" in name:
            assert spill == 0, name
    assert sorted(new) == [(64, "NN", False), (64, "TN", False), (128, "NN", True), (128, "TN", True)], sorted(new)
    for key, (vgpr, spill) in sorted(new.items()):
        print("gemm_bf16_resident_kernel", key, "vgprs", vgpr, "spilled", spill)
        assert spill == 0 and vgpr <= 128, (key, vgpr, spill)
    assert {k: v[0] for k, v in old.items()} == K2B_K2C and not any(v[1] for v in old.values()), old
