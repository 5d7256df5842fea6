"""The kernels of the scatter messages (csrc/elementwise.hip: scatter_msgs_pack_kernel, scatter_msgs_unpack_kernel, each in a
16-byte form and a dword form for tensors whose ld is no multiple of 4) in the code objects inside the built library, read as
tests/test_halo_exact_resources.py reads the exact-width kernels' (no GPU needed): they exist, use no scratch and spill nothing,
and their LDS is the staging they were written with -- 16 KiB for the pack, 32 KiB (and three counters) for the unpack, so that
several workgroups share a compute unit's 160 KiB.  The kernels that were there before keep the resources that test records."""
import pytest

from test_halo_exact_resources import FIELDS, kernels

PACK_LDS = 4096 * 4
UNPACK_LDS = 8192 * 4 + 3 * 4


@pytest.fixture(scope="module")
def ks():
    return kernels()


@pytest.mark.parametrize("stem,lds", [("scatter_msgs_pack_kernel", PACK_LDS), ("scatter_msgs_unpack_kernel", UNPACK_LDS)])
def test_scatter_msgs_kernels_exist_without_scratch_and_within_lds(ks, stem, lds):
    found = {n: v for n, v in ks.items() if stem in n}
    assert len(found) == 2, (stem, sorted(found))          # <true>: 16-byte accesses on the tensor side, <false>: dwords
    for n, v in found.items():
        rec = dict(zip(FIELDS, v))
        print(n, rec, "code bytes", v[-1])
        assert rec["private_segment_fixed_size"] == 0 and rec["vgpr_spill_count"] == 0 and rec["sgpr_spill_count"] == 0, (n, rec)
        assert 0 < rec["group_segment_fixed_size"] <= lds + 16, (n, rec)      # (+16: alignment of the counters behind the staging)
        assert rec["group_segment_fixed_size"] <= 64 * 1024 and rec["vgpr_count"] <= 64, (n, rec)
