"""The form rule of K1's wide (16-byte) bf16 row gather (dory_k1_bf16_wide; csrc/k1_shapes.hpp: k1_rows8_form), asked through
dory_k1_bf16_wide_form (include/dorylus_hip.h): no context, no GPU.  launch_spmm selects its instantiation by the same function.

No form where ld < 64, ld is no multiple of 8, or a pass (ld, or spmm_slab where narrower) is under 64 floats; else by
ch8 = ceil(width / 8): <= 8 (8, 1), <= 16 (16, 1), <= 32 (32, 1), <= 64 (64, 1), <= 96 (32, 3), <= 128 (64, 2), more (64, 3) with
gridDim.y slabs.  Also here: the graphs of tests/k1_bf16_wide_ref.py are what their description says."""
import ctypes as C

import numpy as np
import pytest

import aggregate_ref as ar
import k1_bf16_wide_ref as kr

SLABS = (0, 32, 64, 128, 1024)


@pytest.fixture(scope="module")
def form():
    import dorylus_amd
    return dorylus_amd.k1_bf16_wide_form


def test_the_rule_over_every_row_width_and_slab(form):
    seen = set()
    for ld in range(32, 2049, 32):
        for slab in SLABS:
            got, want = form(ld, slab), kr.form(ld, slab)
            assert got == (want[:2] if want else None), (ld, slab, got, want)
            width = slab if 0 < slab < ld else ld
            assert (got is None) == (ld < 64 or width < 64), (ld, slab, got)
            if got:
                seen.add(got)
    assert sorted(seen) == kr.WIDE_FORMS, sorted(seen)       # every instantiation is reached, nothing else is


def test_lanes_chunks_and_slabs_cover_every_chunk_exactly_once(form):
    """the kernel's own indexing: lane li of a group takes chunks blockIdx.y * lanes * chunks + li + lanes * k, k < chunks, where
    that is below ld / 8"""
    for ld in range(32, 2049, 32):
        for slab in SLABS:
            got = form(ld, slab)
            if not got:
                continue
            lanes, chunks = got
            nchunk = ld // 8
            gridy = -(-nchunk // (lanes * chunks))
            assert gridy == kr.form(ld, slab)[2]
            c = (np.arange(gridy)[:, None, None] * lanes * chunks + np.arange(lanes)[None, :, None] + lanes * np.arange(chunks)[None, None, :]).ravel()
            c = c[c < nchunk]
            assert np.array_equal(np.sort(c), np.arange(nchunk)), (ld, slab, got)
            assert (gridy - 1) * lanes * chunks < nchunk                      # no slab without work
            if gridy == 1 and chunks > 1:
                assert (chunks - 1) * lanes < nchunk, (ld, slab, got)          # no chunk index that no lane uses


def test_the_widths_of_the_gpu_test_take_the_forms_it_names(form):
    for F, slab, want in kr.WIDTHS:
        ld = ar.pad_ld(F)
        assert kr.form(ld, slab) == want, (F, slab)
        assert form(ld, slab) == (want[:2] if want else None), (F, slab)
    assert {w[:2] for _, _, w in kr.WIDTHS if w} == set(kr.WIDE_FORMS)        # one width per instantiation at least
    assert {w[2] for _, s, w in kr.WIDTHS if w and not s} == {1, 2} and [w[2] for _, s, w in kr.WIDTHS if w and s] == [10]


def test_not_multiples_of_eight_null_outputs_and_zeroed_outputs():
    import dorylus_amd
    lib = dorylus_amd.load()
    assert lib.dory_k1_bf16_wide_form(128, 0, None, None) == 1
    g, k = C.c_uint32(7), C.c_uint32(7)
    for ld, slab in ((32, 0), (68, 0), (0, 0), (128, 32), (608, 63)):
        assert lib.dory_k1_bf16_wide_form(ld, slab, C.byref(g), C.byref(k)) == 0, (ld, slab)
        assert (g.value, k.value) == (0, 0)
    assert dorylus_amd.k1_bf16_wide_form(72) == (16, 1) and dorylus_amd.k1_bf16_wide_form(608, 64) == (8, 1)


# ---- the graphs ---------------------------------------------------------------------------------------------------------------
def test_graph203_has_the_planted_degrees_multi_edges_self_loops_and_ghost_ids():
    assert all(kr.N_ROWS % m for m in (4, 8, 16, 32))
    for g0 in (0, 8, 16, 32, 64):
        assert {g0 - 1, g0, g0 + 1} & set(range(200)) <= set(kr.PLANTED) | {-1}
    assert {1, 3, 4, 5} <= set(kr.PLANTED)                   # a batch of four with no tail and tails of 1 and 3; 5 = 4 + 1
    for long_row in (False, True):
        g = kr.graph203("exact", long_row)
        N = int(g["localVtxCnt"])
        assert N == kr.N_ROWS and g["srcGhostCnt"] == kr.N_SRC_GHOSTS and g["dstGhostCnt"] == kr.N_DST_GHOSTS
        for direction, key in (("fwd1", "in"), ("bwd", "out")):
            ptr, idx, val, G = ar.side(g, direction)
            deg = np.diff(ptr.astype(np.int64))
            for v, dg in g["planted"][key].items():
                assert deg[v] == dg, (key, v, dg, deg[v])
            own = np.repeat(np.arange(N), deg)
            assert (idx >= N).any() and idx.max() < N + G                    # ghost ids
            assert (idx == own).any()                                         # self loops
            pairs = own.astype(np.int64) * (N + G) + idx
            assert np.unique(pairs).size < pairs.size                         # multi-edges
            assert (deg.max() == kr.LONG_ROW) == long_row and (long_row or deg.max() < ar.LONG_ROW_CLAMP)
            x, xg = ar.features(g, direction, 8, True)
            ar.exact_ok(ptr, idx, val, g["norm"], x, xg, 1)                   # every partial sum exact in fp32


def test_partition150_has_rows_of_every_kind_and_a_side_nothing_reads():
    g = kr.partition150()
    N = int(g["localVtxCnt"])
    assert (N, int(g["srcGhostCnt"]), int(g["dstGhostCnt"])) == (kr.P_LOCAL, kr.P_GHOSTS, kr.P_GHOSTS)
    ptr, idx, _, _ = ar.side(g, "fwd1")
    own = np.repeat(np.arange(N), np.diff(ptr.astype(np.int64)))
    ghost = np.bincount(own[idx >= N], minlength=N) > 0
    local = np.bincount(own[idx < N], minlength=N) > 0
    assert (ghost & ~local).any() and (local & ~ghost).any() and (ghost & local).any()
    assert 0 < ar.AdjStats(N, ptr, idx).n_boundary < N                        # interior rows and boundary rows: the row split
    ptr, idx, _, _ = ar.side(g, "bwd")
    assert idx.size and (idx < N).all()                                       # ghosts that no out-edge reads
