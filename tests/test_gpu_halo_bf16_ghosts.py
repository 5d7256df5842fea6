"""dory_halo_bf16_ghosts (include/dorylus_hip.h): with dory_halo_bf16_rows on, received bf16 rows stay bf16 in a twin of the ghost
tensor, the aggregation on bf16 rows gathers its ghost rows from the twin, and no bit of any result changes against the switch being
off.  Every comparison is bit for bit; the numpy model is tests/halo_bf16_ghost_ref.py (held against torch by
tests/test_halo_bf16_ghost_reference.py).

  1. the keep kernel through dory_halo_unpack: every width of halo_exact_ref.COLS with ld >= 4, the ghost counts of RECV_ROWS, padded
     and exact rows, direct and non-direct plans; the wire buffer ends a block of bf16 NaN, the twin and the fp32 rows are poisoned
     beforehand; the twin (dory_halo_bf16_ghost_peek) is the numpy model, the state TWIN; a download is the same context's with the
     switch off and leaves BOTH; dory_halo_unpack_tensor sets FP32; a tensor whose raw pointer is out ends BOTH with current raw rows;
  2. epochs over the in-process transport on golden partitions (P = 2, P = 3), new switch on against off with dory_halo_bf16_rows on
     in both, halo_direct_recv 0 / 1 crossed with halo_exact_rows 0 / 1: GCN 41 floats (modes 1 and 2, K1s and K1, overlap 1 and 0),
     GCN 128 floats with the 16-byte gathers, the transform-first order, the GAT prototype (modes 1 and 2, both gat_reuse_nsum); every
     local tensor, weight and gradient the same bits, every ghost tensor the owner's rows rounded where the rule says bf16, the
     statistics what the rule predicts;
  3. state changes between exchange and aggregation (gather mode set to 0, an upload of the ghost tensor, the raw pointer taken before
     the epochs), each against the switch off;
  4. inert and refused cases; in-process ranks that disagree on the switch under a direct plan;
  5. the host transport in two processes under a direct plan (counts and offsets in floats: rows x ld / 2), the scatter transport
     beside it (inert)."""
import ctypes as C
import os
import sys
import traceback

import numpy as np
import pytest

import halo_bf16_ghost_ref as hg
import halo_bf16_ref as hb
import halo_exact_ref as hx
from test_gpu_halo_bf16_rows import GCN_DL, _check_ghosts, _own_views, _same_bits
from test_gpu_halo_exact_rows import _bits, _free_port, _golden, _plan, _raw_rows, _split_ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TWIN_COLS = [c for c in hx.COLS if hx.pad_ld(c) >= 4]
ZERO = dict(landed_direct=0, landed_by_kernel=0, conversions_skipped=0, widened=0)


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _twin(ctx, layer, name):
    """(the rows x ld bf16 of a tensor's twin as uint16, its state)"""
    rows, _, ld, _ = ctx.info(layer, name, ptr=False)
    p, state = ctx.halo_bf16_ghost_peek(layer, name)
    out = np.empty((rows, ld), np.uint16)
    ctx.sync()
    if rows:
        assert p and _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) == 0
    return out, state


def _poison_twin(ctx, layer, name):
    rows, _, ld, _ = ctx.info(layer, name, ptr=False)
    p, _ = ctx.halo_bf16_ghost_peek(layer, name)
    junk = np.full((rows, ld), 0x7FC1, np.uint16)
    ctx.sync()
    if rows:
        assert p and _hip().hipMemcpy(C.c_void_p(p), junk.ctypes.data_as(C.c_void_p), junk.nbytes, 1) == 0


def _twin_bytes(ctx, names=("fg", "fgxw", "bg", "bgg")):
    """what the twins of a context take, from its tensor table: rows x ld x 2 of every named ghost tensor with ld >= 4 but fg@0"""
    total = 0
    for l in range(ctx.L + 1):
        for nm in names:
            try:
                rows, _, ld, _ = ctx.info(l, nm, ptr=False)
            except Exception:
                continue
            if ld >= 4 and not (nm == "fg" and l == 0):
                total += 2 * rows * ld
    return total


def _stats(ctx, keys=("landed_direct", "landed_by_kernel", "conversions_skipped", "widened")):
    s = ctx.halo_bf16_ghosts_stats()
    return {k: s[k] for k in keys}


# ---- 1. the keep kernel through dory_halo_unpack ------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("cols", TWIN_COLS)
def test_unpack_keeps_bf16_rows_in_the_twin(da, cols, direct):
    import aggregate_ref as ar
    import torch
    from helpers import make_ctx
    ld = hx.pad_ld(cols)
    for n_recv in hx.RECV_ROWS[cols]:
        g = ar.graph(hx.graph_name(n_recv))
        ctx = make_ctx(da, g, [4, cols, 2], int(g["globalVtxCnt"]) + 1, node_id=0, num_nodes=2,
                       options={"halo_direct_recv": direct, "gcn_bf16_gather": 2})
        ctx.halo_bf16_rows(1)
        assert ctx.halo_bf16_ghosts_stats() == dict(ZERO, twin_bytes=0) and ctx.halo_bf16_ghost_peek(1, "fg") == (None, hg.FP32)
        for exact in (0, 1):
            ctx.set_option("halo_exact_rows", exact)
            re = hb.row_elems(cols, bool(exact))
            _, slots = _plan(da, ctx, da.FORWARD, 3, n_recv, cols)
            _plan(da, ctx, da.BACKWARD, 3, n_recv, cols + 1000)
            bslots = hx.recv_slots(n_recv, cols + 1000)
            wire = hb.wire_values(n_recv, cols, bool(exact))
            lead = 256
            block = torch.full((lead + n_recv * re,), 0x7FC0, dtype=torch.int16, device="cuda")      # bf16 NaN in front
            if n_recv:
                block[lead:] = torch.from_numpy(wire.view(np.int16)).cuda()
            nan32 = torch.full((max(n_recv * ld, 1),), float("nan"), dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()
            ptr = block.data_ptr() + 2 * lead
            for (layer, name, direction, sl) in ((1, "fg", da.FORWARD, slots), (0, "bg", da.BACKWARD, bslots)):
                unp = np.arange(n_recv) if direct else sl      # (a direct plan stores received row r at ghost row r)
                # the switch off: the widening unpack of dory_halo_bf16_rows (a direct plan: fp32 on the wire, nothing to compare a
                # bf16 buffer with -- the reference is the numpy model alone)
                ctx.halo_bf16_ghosts(0)
                assert ctx.halo_wire_row(1, direction) == ((4, cols if exact else ld) if direct else (2, re))
                want_dl = None
                if not direct:
                    ctx.halo_unpack(1, direction, ptr)
                    want_dl = ctx.download(layer, name)
                ctx.halo_bf16_ghosts(1)
                assert ctx.halo_wire_row(1, direction) == (2, re), (cols, exact, direct)
                assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == _twin_bytes(ctx) >= 2 * 2 * n_recv * ld
                # poison: NaN into every fp32 element (a padded fp32 row carries its padding) and into the twin
                if not exact:
                    ctx.halo_unpack_tensor(layer, name, direction, nan32.data_ptr())
                _poison_twin(ctx, layer, name)
                assert ctx.halo_bf16_ghost_peek(layer, name)[1] == hg.FP32
                before = _stats(ctx)
                staged = ctx.get_option("halo_staged_recvs")
                ctx.halo_unpack(1, direction, ptr)
                got, state = _twin(ctx, layer, name)
                want = hg.keep(np.full((n_recv, ld), 0x7FC1, np.uint16), unp, wire, cols, bool(exact))
                assert np.array_equal(got, want), (cols, exact, direct, n_recv, name, "twin rows")
                assert (got[:, re:] == 0).all() and state == hg.TWIN
                assert _stats(ctx) == dict(before, landed_by_kernel=before["landed_by_kernel"] + 1) and ctx.get_option("halo_staged_recvs") == staged
                # a download widens: the caller's row order, the switch-off bits; then both copies are current
                dl = ctx.download(layer, name)
                model = np.zeros((n_recv, ld), np.float32)
                model[sl] = hg.widen(want)[np.arange(n_recv)] if direct else hg.widen(want)[sl]
                assert np.array_equal(_bits(dl), _bits(model[:, :cols])), (cols, exact, direct, n_recv, name, "download")
                if want_dl is not None:
                    assert np.array_equal(_bits(dl), _bits(want_dl)), (cols, exact, n_recv, name, "download against the switch off")
                assert ctx.halo_bf16_ghost_peek(layer, name)[1] == hg.BOTH and _stats(ctx)["widened"] == before["widened"] + 1
                ctx.download(layer, name)
                assert _stats(ctx)["widened"] == before["widened"] + 1          # (BOTH: nothing to widen)
                # dory_halo_unpack_tensor writes fp32 rows
                if not exact:
                    ctx.halo_unpack_tensor(layer, name, direction, nan32.data_ptr())
                    assert ctx.halo_bf16_ghost_peek(layer, name)[1] == hg.FP32
        # the raw pointer handed out: the fp32 rows follow the twin at once (all ld elements: zeros in the padding), state BOTH
        if n_recv:
            ctx.halo_unpack(1, da.FORWARD, ptr)
            assert ctx.halo_bf16_ghost_peek(1, "fg")[1] == hg.TWIN
            before = _stats(ctx)
            raw = _raw_rows(ctx, 1, "fg")                      # (dory_tensor_info widens before it hands the pointer out)
            assert ctx.halo_bf16_ghost_peek(1, "fg")[1] == hg.BOTH and _stats(ctx)["widened"] == before["widened"] + 1
            tw, _ = _twin(ctx, 1, "fg")
            assert np.array_equal(_bits(raw), _bits(hg.widen(tw)))
            _poison_twin(ctx, 1, "fg")
            ctx.halo_unpack(1, da.FORWARD, ptr)
            assert ctx.halo_bf16_ghost_peek(1, "fg")[1] == hg.BOTH and _stats(ctx)["widened"] == before["widened"] + 1
            tw2, _ = _twin(ctx, 1, "fg")
            assert np.array_equal(tw2, tw) and np.array_equal(_bits(_raw_rows(ctx, 1, "fg")), _bits(hg.widen(tw)))
        # off: the twins go, after the one that alone is current has been widened
        ctx.halo_unpack(1, da.BACKWARD, ptr)
        tw, state = _twin(ctx, 0, "bg")
        assert state == hg.TWIN
        w0 = _stats(ctx)["widened"]
        ctx.halo_bf16_ghosts(0)
        assert ctx.halo_bf16_ghost_peek(0, "bg") == (None, hg.FP32) and ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0
        assert _stats(ctx)["widened"] == w0 + 1
        sl = hx.recv_slots(n_recv, cols + 1000)
        model = np.zeros((n_recv, ld), np.float32)
        model[sl] = hg.widen(tw)[np.arange(n_recv)] if direct else hg.widen(tw)[sl]
        assert np.array_equal(_bits(ctx.download(0, "bg")), _bits(model[:, :cols]))
        ctx.close()


# ---- 2. epochs over the in-process transport ---------------------------------------------------------------------------------
def _keep(setup, kept):
    """run_local closes its contexts: read the statistics of every rank just before that"""
    def wrapped(ctx, r, g):
        setup(ctx, r, g)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"ghosts": ctx.halo_bf16_ghosts_stats(), "twin_bytes": _twin_bytes(ctx, ("fg", "fgxw", "bg", "bgg", "fg_z", "bg_d")), "bf16": ctx.halo_bf16_rows_stats(),
                           "staged": ctx.get_option("halo_staged_recvs"), "direct": ctx.get_option("halo_direct_recvs"),
                           "gat_gathers": ctx.gat_bf16_gather_stats()}
                try:
                    kept[r]["gcn_gathers"] = ctx.get_option("gcn_bf16_gathers_k1s") + ctx.get_option("gcn_bf16_gathers_k1")
                    kept[r]["wide"] = ctx.get_option("gcn_bf16_gathers_k1s_wide")
                except Exception:              # (keys of the GCN model)
                    kept[r]["gcn_gathers"] = kept[r]["wide"] = None
            close()
        ctx.close = closing
    return wrapped


def _gcn_run(da, case, dims, epochs, opts, ghosts, dl, rows=1, seed=5, after=None):
    from local_ranks import run_local
    pobjs, parts = case() if callable(case) else _golden(da, case)
    V, L = len(parts), len(dims) - 1
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]

    def setup(ctx, r, g):
        if g["localVtxCnt"]:
            ctx.upload(0, "x", X[g["localToGlobal"]])
        if g["srcGhostCnt"]:
            ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), dims[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
        ctx.halo_bf16_rows(rows)
        ctx.halo_bf16_ghosts(ghosts)
        if opts.get("gcn_transform_first"):
            assert all(ctx.transform_first_layer(l) for l in range(L)), "the transform-first order is not active"
        if after:
            after(ctx, r, g)
    kept = {}
    out = run_local(da, pobjs, parts, dims, da.GCN, epochs, _keep(setup, kept), opts, downloads=dl)
    out["views"] = _own_views(pobjs)
    return out, kept


def _check_gcn_stats(kon, koff, views, epochs, mode, direct, cols, exact, what, downloads=1):
    """per rank, from the rule: one forward and one backward exchange an epoch; forward ships bf16 (mode >= 1), backward with mode 2"""
    nbf = 2 if mode == 2 else 1
    lands = hg.lands_directly(direct, cols, bool(exact))
    for r, g in enumerate(views):
        have = int(g["srcGhostCnt"]) > 0
        assert have == (int(g["dstGhostCnt"]) > 0)
        s = kon[r]["ghosts"]
        assert s["landed_direct"] == (epochs * nbf if lands else 0) and s["landed_by_kernel"] == (0 if lands else epochs * nbf), (what, r, s)
        assert s["conversions_skipped"] == (epochs * nbf if have else 0), (what, r, s, kon[r]["gcn_gathers"])
        assert s["widened"] == (downloads * nbf if have else 0), (what, r, s)
        assert s["twin_bytes"] == kon[r]["twin_bytes"] and (s["twin_bytes"] > 0) == have, (what, r, s)
        assert kon[r]["bf16"][0] == epochs * nbf and kon[r]["bf16"][2] == epochs * (2 - nbf), (what, r, kon[r]["bf16"])
        if direct:      # without the new switch a direct plan keeps fp32; with it, what lands directly moves no row through a staged receive
            assert koff[r]["bf16"][0] == 0 and koff[r]["bf16"][2] == 2 * epochs, (what, r, koff[r]["bf16"])
            fp32_direct = (2 - nbf) * epochs if not exact or cols % 32 == 0 else 0
            assert kon[r]["direct"] == s["landed_direct"] + fp32_direct and kon[r]["staged"] == 2 * epochs - kon[r]["direct"], (what, r, kon[r])
        else:
            assert koff[r]["bf16"] == kon[r]["bf16"] and kon[r]["staged"] == 2 * epochs and kon[r]["direct"] == 0
        assert {k: koff[r]["ghosts"][k] for k in ZERO} == ZERO and koff[r]["ghosts"]["twin_bytes"] == 0, (what, r, koff[r]["ghosts"])


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("exact", [0, 1])
def test_local_transport_gcn_epochs_bf16_ghosts_same_bits(da, case, mode, direct, exact):
    """three epochs with layers of 41 floats: K1s in two launches and K1, overlap on and off; new switch on against off"""
    dims, epochs = [20, 41, 6], 3
    for variant in ({"spmm_blk_nb": 8}, {"spmm_variant": 0}):
        for overlap in (1, 0):
            opts = dict(variant, halo_overlap=overlap, halo_exact_rows=exact, halo_direct_recv=direct, gcn_bf16_gather=mode)
            what = (case, mode, direct, exact, variant, overlap)
            on, kon = _gcn_run(da, case, dims, epochs, opts, 1, GCN_DL)
            off, koff = _gcn_run(da, case, dims, epochs, opts, 0, GCN_DL)
            _same_bits(on, off, what)
            bwd = mode == 2
            _check_ghosts(on, [((1, "fg"), (0, "h"), "srcGhost", True), ((0, "bg"), (1, "grad"), "dstGhost", bwd)], what)
            _check_ghosts(off, [((1, "fg"), (0, "h"), "srcGhost", not direct), ((0, "bg"), (1, "grad"), "dstGhost", bwd and not direct)], what)
            _check_gcn_stats(kon, koff, on["views"], epochs, mode, direct, 41, exact, what)


@pytest.mark.parametrize("direct", [0, 1])
@pytest.mark.parametrize("exact", [0, 1])
def test_local_transport_gcn_wide_gathers_read_the_twin(da, direct, exact):
    """layers of 128 floats with gcn_bf16_wide = 1: the 16-byte gathers of K1s read the twin"""
    dims, epochs = [20, 128, 6], 3
    opts = {"spmm_blk_nb": 8, "gcn_bf16_wide": 1, "gcn_bf16_gather": 2, "halo_exact_rows": exact, "halo_direct_recv": direct}
    for case in ("parts_toy60_p2", "parts_toy40_p3_empty"):
        what = ("wide", case, direct, exact)
        on, kon = _gcn_run(da, case, dims, epochs, opts, 1, GCN_DL)
        off, koff = _gcn_run(da, case, dims, epochs, opts, 0, GCN_DL)
        _same_bits(on, off, what)
        _check_ghosts(on, [((1, "fg"), (0, "h"), "srcGhost", True), ((0, "bg"), (1, "grad"), "dstGhost", True)], what)
        _check_gcn_stats(kon, koff, on["views"], epochs, 2, direct, 128, exact, what)
        assert any(k["wide"] > 0 for k in kon.values()) and [k["wide"] for k in kon.values()] == [k["wide"] for k in koff.values()], (what, kon)


@pytest.mark.parametrize("direct", [0, 1])
def test_local_transport_gcn_transform_first_bf16_ghosts_same_bits(da, direct):
    """the transform-first order on partitions built from directed records (P = 2): xw -> fgxw forward, g -> bgg backward"""
    dims, epochs = [33, 25, 6, 3], 3
    rng = np.random.default_rng(17)
    V, E = 240, 2600
    es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
    ed[:200] = 7
    es[200:400] = 13
    pv = (rng.permutation(V) % 2).astype(np.int32)
    case = lambda: ([da.Partition.build(es.astype(np.uint32), ed.astype(np.uint32), pv, r, 2) for r in range(2)], pv)
    dl = [(l, nm) for l in range(3) for nm in ("z", "bgg")] + [(l, nm) for l in (1, 2) for nm in ("xw", "fgxw")] + [(l, nm) for l in (0, 1) for nm in ("h", "aTg")]
    for mode in (1, 2):
        for exact in (0, 1):
            opts = {"spmm_blk_nb": 8, "gcn_transform_first": 2, "halo_exact_rows": exact, "gcn_bf16_gather": mode, "halo_direct_recv": direct}
            what = ("transform first", mode, exact, direct)
            on, kon = _gcn_run(da, case, dims, epochs, opts, 1, dl)
            off, koff = _gcn_run(da, case, dims, epochs, opts, 0, dl)
            ref, _ = _gcn_run(da, case, dims, epochs, opts, 0, dl, rows=0)            # fp32 on every wire
            _same_bits(on, off, what)
            _check_ghosts(on, [((l, "fgxw"), (l, "xw"), "srcGhost", True) for l in (1, 2)], what)
            for r in range(2):      # g is a temporary: the backward ghost rows against the fp32 payload's, rounded where the rule says bf16
                for l in range(3):
                    want = ref["tensors"][r][(l, "bgg")]
                    want = hb.rounded(want) if mode == 2 else want
                    assert np.array_equal(_bits(on["tensors"][r][(l, "bgg")]), _bits(want)), (what, r, l, "bgg")
            for r in range(2):
                s, b = kon[r]["ghosts"], kon[r]["bf16"]
                assert s["landed_direct"] + s["landed_by_kernel"] == b[0] > 0, (what, r, s, b)
                # widths 25 and 6 (ld 32) and 3 (ld 32): exact rows never fill a twin row, padded ones always do
                assert (s["landed_by_kernel"] == 0) == bool(direct and not exact), (what, r, s)
                assert s["conversions_skipped"] == b[0], (what, r, s, b)        # every bf16 exchange is read by one aggregation on bf16 rows
                assert {k: koff[r]["ghosts"][k] for k in ZERO} == ZERO
                assert (koff[r]["bf16"][0] == 0) == bool(direct)


def _gat_run(da, case, dims, epochs, opts, ghosts, dl, mode, seed=11):
    from local_ranks import run_local
    pobjs, parts = _golden(da, case)
    V, L = len(parts), len(dims) - 1
    rng = np.random.default_rng(seed)
    H0 = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32) for l in range(L)]
    As = [(rng.standard_normal((dims[l + 1], 1)) / 2).astype(np.float32) for l in range(L)]

    def setup(ctx, r, g):
        if g["localVtxCnt"]:
            ctx.upload(0, "h", H0[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l in range(L):
            ctx.weight_set(l, "w", Ws[l])
            ctx.weight_set(l, "a_i", As[l])
        ctx.gat_bf16_gather(mode)
        ctx.halo_bf16_rows(1)
        ctx.halo_bf16_ghosts(ghosts)
    kept = {}
    out = run_local(da, pobjs, parts, dims, da.GAT, epochs, _keep(setup, kept), opts, downloads=dl)
    out["views"] = _own_views(pobjs)
    return out, kept


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("direct", [0, 1])
def test_local_transport_gat_prototype_bf16_ghosts_same_bits(da, case, mode, direct):
    """the GAT prototype: z -> fg_z forward (mode >= 1), grad -> bg_d backward (mode 2), both gat_reuse_nsum settings"""
    dims, epochs, L = [20, 16, 6], 3, 2
    dl = [(l, nm) for l in range(L) for nm in ("z", "ah", "grad", "aTg", "fg_z", "bg_d", "nsum")]
    nbf = 2 if mode == 2 else 1
    for reuse in (1, 0):
        for exact in (0, 1):
            opts = {"spmm_blk_nb": 8, "gat_reuse_nsum": reuse, "halo_exact_rows": exact, "halo_direct_recv": direct}
            what = (case, mode, direct, reuse, exact)
            on, kon = _gat_run(da, case, dims, epochs, opts, 1, dl, mode)
            off, koff = _gat_run(da, case, dims, epochs, opts, 0, dl, mode)
            _same_bits(on, off, what)
            pairs = lambda f, b: [((l, "fg_z"), (l, "z"), "srcGhost", f) for l in range(L)] + [((l, "bg_d"), (l, "grad"), "dstGhost", b) for l in range(L)]
            _check_ghosts(on, pairs(True, mode == 2), what)
            _check_ghosts(off, pairs(not direct, mode == 2 and not direct), what)
            lands = bool(direct and not exact)         # 16 and 6 floats in an ld of 32: only padded rows fill a twin row
            for r, g in enumerate(on["views"]):
                have = int(g["srcGhostCnt"]) > 0
                s, gs = kon[r]["ghosts"], kon[r]["gat_gathers"]
                assert s["landed_direct"] == (epochs * L * nbf if lands else 0) and s["landed_by_kernel"] == (0 if lands else epochs * L * nbf), (what, r, s)
                # every aggregation on bf16 rows reads fg_z or bg_d, which the rule landed as bf16 whenever it runs on bf16 rows
                assert s["conversions_skipped"] == (gs["k1s"] + gs["k1"] if have else 0) and (not have or s["conversions_skipped"] >= epochs * L * nbf), (what, r, s, gs)
                assert gs == koff[r]["gat_gathers"]
                assert s["widened"] == (L * nbf if have else 0), (what, r, s)
                assert kon[r]["bf16"][0] == epochs * L * nbf and (koff[r]["bf16"][0] == 0) == bool(direct)
                assert {k: koff[r]["ghosts"][k] for k in ZERO} == ZERO


# ---- 3. state changes between exchange and aggregation -----------------------------------------------------------------------
def _pair(da, ghosts, direct, raw_first=False, mode=2):
    """two ranks of parts_toy60_p2 driven stage by stage from this thread: GCN [20, 41, 6], h@0 -> fg@1"""
    pobjs, parts = _golden(da, "parts_toy60_p2")
    gs = _own_views(pobjs)                     # (copies: a view's arrays live in its partition object)
    ctxs = []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GCN, [20, 41, 6], len(parts), r, 2)
        for k, v in (("spmm_blk_nb", 8), ("local_timeout_ms", 2000), ("gcn_bf16_gather", mode), ("halo_direct_recv", direct)):
            ctx.set_option(k, v)
        part.upload(ctx, parts)
        ctx.preallocate()
        ctx.halo_bf16_rows(1)
        ctx.halo_bf16_ghosts(ghosts)
        if raw_first:
            ctx.info(1, "fg")
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    return ctxs, gs


def _exchange(ctxs, H):
    for r, c in enumerate(ctxs):
        c.upload(0, "h", H[r])
    for c in ctxs:
        c.halo_exchange(1, 0)
    for c in ctxs:
        c.sync()


@pytest.mark.parametrize("direct", [0, 1])
def test_state_changes_between_exchange_and_aggregation(da, direct):
    rng = np.random.default_rng(23)
    res = {}
    for ghosts in (1, 0):
        ctxs, gs = _pair(da, ghosts, direct)
        H = [rng.uniform(-1, 1, (int(g["localVtxCnt"]), 41)).astype(np.float32) for g in gs] if ghosts else res["H"]
        U = [rng.uniform(-1, 1, (int(g["srcGhostCnt"]), 41)).astype(np.float32) for g in gs] if ghosts else res["U"]
        res["H"], res["U"] = H, U
        out = {}
        # (a) an aggregation on bf16 rows reads the twin
        _exchange(ctxs, H)
        for r, c in enumerate(ctxs):
            assert c.halo_bf16_ghost_peek(1, "fg")[1] == (hg.TWIN if ghosts else hg.FP32)
            c.aggregate(1, 0)
            out[("bf16", r)] = c.download(1, "ah")
            assert _stats(c) == (dict(ZERO, conversions_skipped=1, **{"landed_direct" if direct else "landed_by_kernel": 1}) if ghosts else ZERO), (r, _stats(c))
            assert c.halo_bf16_ghost_peek(1, "fg")[1] == (hg.TWIN if ghosts else hg.FP32)
        # (b) gather mode 0 after the exchange: an fp32 aggregation of the widened rows
        for r, c in enumerate(ctxs):
            c.set_option("gcn_bf16_gather", 0)
            c.aggregate(1, 0)
            out[("mode0", r)] = c.download(1, "ah")
            assert c.halo_bf16_ghost_peek(1, "fg")[1] == (hg.BOTH if ghosts else hg.FP32) and _stats(c)["widened"] == ghosts
            c.set_option("gcn_bf16_gather", 2)
            out[("fg", r)] = c.download(1, "fg")
            assert _stats(c)["widened"] == ghosts
        # (c) an upload of the ghost tensor after the exchange: those rows are the ones gathered
        _exchange(ctxs, H)
        for r, c in enumerate(ctxs):
            skipped = _stats(c)["conversions_skipped"]
            c.upload(1, "fg", U[r])
            assert c.halo_bf16_ghost_peek(1, "fg")[1] == hg.FP32
            c.aggregate(1, 0)
            out[("upload", r)] = c.download(1, "ah")
            assert _stats(c)["conversions_skipped"] == skipped
            assert not np.array_equal(_bits(out[("upload", r)]), _bits(out[("bf16", r)]))
            assert np.array_equal(_bits(c.download(1, "fg")), _bits(U[r]))
        for c in ctxs:
            c.close()
        res[ghosts] = out
    assert set(res[1]) == set(res[0])
    for k in res[1]:
        a, b = res[1][k], res[0][k]
        if k[0] == "mode0" and direct:
            continue                           # (without the new switch a direct plan ships fp32: that fp32 aggregation reads unrounded ghost rows)
        if k[0] == "fg" and direct:
            b = hb.rounded(b)
        assert np.array_equal(_bits(a), _bits(b)), (direct, k)
    for r in (0, 1):       # the fp32 aggregation saw rounded rows where bf16 travelled, so only there is it the bf16 aggregation's neighbour
        assert not np.array_equal(_bits(res[1][("mode0", r)]), _bits(res[1][("bf16", r)]))


@pytest.mark.parametrize("direct", [0, 1])
def test_raw_pointer_taken_before_the_epochs_keeps_fp32_rows_current(da, direct):
    rng = np.random.default_rng(29)
    res = {}
    Hs = None
    for ghosts in (1, 0):
        ctxs, gs = _pair(da, ghosts, direct, raw_first=True)
        Hs = Hs or [[rng.uniform(-1, 1, (int(g["localVtxCnt"]), 41)).astype(np.float32) for g in gs] for _ in range(3)]
        out = {}
        for e in range(3):
            _exchange(ctxs, Hs[e])
            for r, c in enumerate(ctxs):
                assert c.halo_bf16_ghost_peek(1, "fg")[1] == (hg.BOTH if ghosts else hg.FP32), (e, r)
                out[("raw", e, r)] = _raw_rows(c, 1, "fg")
                if ghosts:
                    tw, _ = _twin(c, 1, "fg")
                    assert np.array_equal(_bits(out[("raw", e, r)]), _bits(hg.widen(tw))), (e, r)
                c.aggregate(1, 0)
                out[("ah", e, r)] = c.download(1, "ah")
        for c in ctxs:
            s = _stats(c)
            assert s == (dict(ZERO, **{"landed_direct" if direct else "landed_by_kernel": 3}) if ghosts else ZERO), s      # (raw pointer out: converted from fp32)
            c.close()
        res[ghosts] = out
    for k in res[1]:
        b = res[0][k]
        if k[0] == "raw" and direct:
            b = hb.rounded(b)
        assert np.array_equal(_bits(res[1][k]), _bits(b)), (direct, k)


# ---- 4. inert and refused cases ---------------------------------------------------------------------------------------------------
def _inert(kon, koff, what):
    for r in kon:
        assert {k: kon[r]["ghosts"][k] for k in ZERO} == ZERO, (what, r, kon[r]["ghosts"])
        assert kon[r]["bf16"] == koff[r]["bf16"] and kon[r]["staged"] == koff[r]["staged"] and kon[r]["direct"] == koff[r]["direct"], (what, r)


@pytest.mark.parametrize("direct", [0, 1])
def test_gather_mode_0_and_rows_switch_off_are_inert(da, direct):
    dims, epochs = [20, 41, 6], 2
    pairs = [((1, "fg"), (0, "h"), "srcGhost", False), ((0, "bg"), (1, "grad"), "dstGhost", False)]
    for mode, rows in ((0, 1), (2, 0)):
        poisoned = []

        def after(ctx, r, g):      # no twin is written: what they held before the epochs is what they hold after them
            for layer, nm in ((1, "fg"), (0, "bg")):
                if ctx.info(layer, nm, ptr=False)[0]:
                    _poison_twin(ctx, layer, nm)
                    poisoned.append((ctx, layer, nm))
            close = ctx.close

            def closing():
                if ctx.h:
                    for c2, layer, nm in poisoned:
                        if c2 is ctx:
                            tw, state = _twin(ctx, layer, nm)
                            assert state == hg.FP32 and (tw == 0x7FC1).all(), (mode, rows, r, nm)
                close()
            ctx.close = closing
        opts = {"spmm_blk_nb": 8, "gcn_bf16_gather": mode, "halo_direct_recv": direct}
        on, kon = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 1, GCN_DL, rows=rows, after=after)
        off, koff = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 0, GCN_DL, rows=rows)
        assert len(poisoned) == 4
        _same_bits(on, off, (mode, rows, direct), ghosts_too=True)
        _check_ghosts(on, pairs, (mode, rows, direct))
        _inert(kon, koff, (mode, rows, direct))
        assert all(k["ghosts"]["twin_bytes"] > 0 for k in kon.values())


def test_multi_head_gat_has_no_twins(da):
    from test_gpu_halo_bf16_rows import _gat_run as mh_run
    dims, heads = [20, 128, 6], [8, 1]
    dl = [(l, nm) for l in range(2) for nm in ("z", "o", "dz", "fg_z", "bg_do", "bg_st")] + [(1, "logits")]
    seen = {}

    def with_switch(on):
        import dorylus_amd._lib as lib
        orig = lib.Context.halo_bf16_rows

        def both(self, v=True):        # (the runner of the bf16-rows tests sets that switch last: the new one goes with it)
            orig(self, v)
            self.halo_bf16_ghosts(on)
            seen[on] = self.halo_bf16_ghosts_stats()
        lib.Context.halo_bf16_rows = both
        try:
            return mh_run(da, da.GATMH, "parts_toy60_p2", dims, 1, {"spmm_blk_nb": 8}, 1, dl, heads=heads)
        finally:
            lib.Context.halo_bf16_rows = orig
    on, kon = with_switch(1)
    off, koff = with_switch(0)
    _same_bits(on, off, "8-head GAT", ghosts_too=True)
    assert seen[1] == dict(ZERO, twin_bytes=0) and seen[0] == dict(ZERO, twin_bytes=0)
    for r in kon:
        assert kon[r]["bf16"] == koff[r]["bf16"] and kon[r]["bf16"][:2] == (0, 0)


def test_refused_arguments(da):
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="error -1.*halo_bf16_ghosts"):
        c.halo_bf16_ghosts(1)                          # before dory_configure
    c.configure(da.GCN, [4, 41, 2], 100, 0, 2)
    with pytest.raises(da.DoryError, match="error -1.*halo_bf16_ghosts.*dory_preallocate"):
        c.halo_bf16_ghosts(1)                          # before dory_preallocate
    c.close()
    ctx = _split_ctx(da, 41, 3)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="error -1.*halo_bf16_ghosts"):
            ctx.halo_bf16_ghosts(bad)
    with pytest.raises(da.DoryError, match="error -1.*halo_bf16_ghost_peek"):
        ctx.halo_bf16_ghost_peek(0, "nothing")
    ctx.halo_bf16_ghosts(1)
    ctx.halo_bf16_ghosts(1)                            # again: nothing new
    assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == _twin_bytes(ctx) == 2 * 3 * 2 * (64 + 32)      # fg@1, bg@0 (41 -> 64); fgxw@1, bgg@1 (2 -> 32)
    assert ctx.halo_bf16_ghost_peek(0, "fg") == (None, hg.FP32) and ctx.halo_bf16_ghost_peek(0, "h") == (None, hg.FP32)      # file-loaded fg@0, a local tensor
    ctx.preallocate()                                  # new tensors, new twins
    assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == _twin_bytes(ctx) and ctx.halo_bf16_ghost_peek(1, "fg")[0]
    ctx.halo_bf16_ghosts(0)
    assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0
    ctx.close()
    one = _split_ctx(da, 1, 3)                         # a one-column tensor gets no twin
    one.halo_bf16_ghosts(1)
    assert one.halo_bf16_ghosts_stats()["twin_bytes"] == _twin_bytes(one) and one.halo_bf16_ghost_peek(1, "fg") == (None, hg.FP32)
    one.close()


def test_local_transport_refuses_ranks_that_disagree_under_a_direct_plan(da):
    """rank 0 with the new switch on, rank 1 off, a direct plan: rank 0 would ship bf16, rank 1 fp32 -- DORY_ERR_COMM on either rank
    before anything is enqueued or counted; fixed, the exchange runs.  Without a direct plan the same disagreement is none: both ship bf16"""
    rng = np.random.default_rng(3)
    for direct in (1, 0):
        ctxs, gs = _pair(da, 1, direct)
        ctxs[1].halo_bf16_ghosts(0)
        H = [rng.uniform(-1, 1, (int(g["localVtxCnt"]), 41)).astype(np.float32) for g in gs]
        for r, c in enumerate(ctxs):
            c.upload(0, "h", H[r])
        if direct:
            for r in (0, 1):
                before = ctxs[r].halo_bf16_rows_stats(), _stats(ctxs[r])
                with pytest.raises(da.DoryError, match=r"error -4.*dory_halo_bf16_rows differs.*rank %d ships %s rows, rank %d %s rows.*dory_halo_bf16_ghosts"
                                   % (r, "bf16" if r == 0 else "fp32", 1 - r, "fp32" if r == 0 else "bf16")):
                    ctxs[r].halo_exchange(1, da.FORWARD)
                assert (ctxs[r].halo_bf16_rows_stats(), _stats(ctxs[r])) == before
            ctxs[1].halo_bf16_ghosts(1)
        _exchange(ctxs, H)
        g2row = {int(gv): H[r][i] for r in (0, 1) for i, gv in enumerate(gs[r]["localToGlobal"])}
        for r in (0, 1):
            want = hb.rounded(np.stack([g2row[int(gv)] for gv in gs[r]["srcGhost"]]))
            assert np.array_equal(_bits(ctxs[r].download(1, "fg")), _bits(want)), (direct, r)
            assert ctxs[r].halo_bf16_rows_stats()[0] == 1
        for c in ctxs:
            c.close()


# ---- 5. the host transport and the scatter transport, two processes -----------------------------------------------------------
def _worker(rank, world, port, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "oracle"))
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch
        import torch.distributed as dist
        import dorylus_amd as da
        dist.init_process_group("gloo", rank=rank, world_size=world)
        dims = [20, 41, 6]
        pobjs, parts = _golden(da, "parts_toy60_p2")
        part, g = pobjs[rank], pobjs[rank].view()
        V, L = len(parts), len(dims) - 1
        rng = np.random.default_rng(9)
        X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
        labels = rng.integers(0, dims[-1], V).astype(np.uint32)
        Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]

        def allreduce(buf):
            t = torch.from_numpy(buf.copy())
            dist.all_reduce(t)
            buf[:] = t.numpy()

        def run(transport, on):
            ctx = da.Context(0)
            ctx.configure(da.GCN, dims, V, rank, world)
            for k, v in (("spmm_blk_nb", 8), ("halo_direct_recv", 1), ("gcn_bf16_gather", 2)):
                ctx.set_option(k, v)
            part.upload(ctx, parts)
            ctx.preallocate()
            ctx.upload(0, "x", X[g["localToGlobal"]])
            if g["srcGhostCnt"]:
                ctx.upload(0, "fg", X[g["srcGhost"]].reshape(g["srcGhostCnt"], dims[0]))
            ctx.labels_upload(labels[g["localToGlobal"]])
            for l, W in enumerate(Ws):
                ctx.weight_set(l, "w", W)
            ctx.adam_config(0.01)
            ctx.halo_bf16_rows(1)
            ctx.halo_bf16_ghosts(on)
            seen = []

            def alltoallv(send, sc, so, recv, rc, ro):
                seen.append(tuple([int(x) for x in a] for a in (sc, so, rc, ro)))
                reqs, keep = [], []
                for p in range(world):
                    if p == rank:
                        continue
                    if rc[p]:
                        t = torch.empty(int(rc[p]), dtype=torch.float32)
                        keep.append((t, int(ro[p]), int(rc[p])))
                        reqs.append(dist.irecv(t, p))
                    if sc[p]:
                        reqs.append(dist.isend(torch.from_numpy(send[int(so[p]):int(so[p] + sc[p])].copy()), p))
                for r_ in reqs:
                    r_.wait()
                for t, o, n in keep:
                    recv[o:o + n] = t.numpy()

            def exchange(msgs):
                out = [[] for _ in range(world)]
                for peer, m in msgs:
                    out[peer].append(m.tobytes())
                every = [None] * world
                dist.all_gather_object(every, out)
                seen.append(sum(len(m) for row in out for m in row))
                mine = [m for s_ in range(world) if s_ != rank for m in every[s_][rank]]
                if mine:
                    ctx.scatter_msgs_deliver(mine)
            if transport == "scatter":
                ctx.set_scatter_transport(exchange, allreduce, 4096)
            else:
                ctx.set_host_transport(alltoallv, allreduce)
            eng = da.NativeEngine(ctx)
            eng.run(1)
            ctx.sync()
            res = {"seen": seen, "stats": ctx.halo_bf16_rows_stats(), "wire": ctx.halo_wire_row(1, da.FORWARD),
                   "states": [ctx.halo_bf16_ghost_peek(1, "fg")[1], ctx.halo_bf16_ghost_peek(0, "bg")[1]],
                   "recvs": (ctx.get_option("halo_direct_recvs"), ctx.get_option("halo_staged_recvs")), "tensors": {}, "W": [], "dW": []}
            for l, nm in ((0, "ah"), (1, "ah"), (0, "h"), (0, "aTg"), (1, "grad"), (1, "fg"), (0, "bg")):
                if ctx.info(l, nm, ptr=False)[0]:
                    res["tensors"][(l, nm)] = ctx.download(l, nm)
            for l in range(L):
                res["W"].append(ctx.weight_get(l))
                res["dW"].append(ctx.weight_grad_get(l))
            res["ghosts"] = ctx.halo_bf16_ghosts_stats()          # (after the downloads: they widen)
            res["states_after"] = [ctx.halo_bf16_ghost_peek(1, "fg")[1], ctx.halo_bf16_ghost_peek(0, "bg")[1]]
            eng.close()
            ctx.close()
            return res
        out = {(t, on): run(t, on) for t in ("host", "scatter") for on in (1, 0)}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_host_transport_direct_plan_lands_in_the_twin_and_scatter_transport_inert():
    """two processes on one GPU, the bytes over gloo, plans made with halo_direct_recv = 1.  Host transport: with the new switch the
    callback is given rows x ld / 2 = rows x 32 floats (without it rows x 64: fp32), the H2D copy lands in the twin, the epoch's bits
    are the switch-off bits and the ghost rows arrive rounded.  Scatter transport: the same message bytes, no twin written."""
    import torch.multiprocessing as mp
    world = 2
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = _free_port()
    procs = [ctxm.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = []
    try:
        for _ in range(world):
            res.append(q.get(timeout=600))
    finally:
        for p in procs:
            p.join(timeout=60)
            if p.is_alive():
                p.kill()
    res.sort(key=lambda t: t[0])
    for rank, r in res:
        assert isinstance(r, dict), f"rank {rank} failed:\n{r}"
    res = [r for _, r in res]

    def same(a, b, what, skip=()):
        assert set(a["tensors"]) == set(b["tensors"])
        for k in a["tensors"]:
            if k not in skip:
                assert np.array_equal(_bits(a["tensors"][k]), _bits(b["tensors"][k])), (what, k)
        for l in range(2):
            assert np.array_equal(_bits(a["W"][l]), _bits(b["W"][l])) and np.array_equal(_bits(a["dW"][l]), _bits(b["dW"][l])), (what, l)
    for rank in (0, 1):
        on, off = res[rank][("host", 1)], res[rank][("host", 0)]
        assert len(on["seen"]) == len(off["seen"]) == 2
        for c_on, c_off in zip(on["seen"], off["seen"]):
            for a_on, a_off in zip(c_on, c_off):
                assert all(x % 64 == 0 for x in a_off), (rank, a_off)
                assert a_on == [x // 64 * 32 for x in a_off], (rank, a_on, a_off)
        rows = sum(sum(c[0]) for c in off["seen"]) // 64
        assert rows > 0 and on["stats"] == (2, rows * 128, 0) and off["stats"] == (0, 0, 2), (rank, on["stats"], off["stats"])
        assert on["wire"] == (2, 64) and off["wire"] == (4, 64)
        # both exchanges landed in the twins themselves: no staged receive; each twin read by one aggregation, widened by one download
        assert {k: on["ghosts"][k] for k in ZERO} == dict(landed_direct=2, landed_by_kernel=0, conversions_skipped=2, widened=2), (rank, on["ghosts"])
        assert {k: off["ghosts"][k] for k in ZERO} == ZERO and off["ghosts"]["twin_bytes"] == 0
        assert on["recvs"] == (2, 0) and off["recvs"] == (2, 0) and on["states"] == [hg.TWIN, hg.TWIN] and on["states_after"] == [hg.BOTH, hg.BOTH] and off["states"] == off["states_after"] == [hg.FP32, hg.FP32]
        same(on, off, ("host", rank), skip=((1, "fg"), (0, "bg")))
        for k in ((1, "fg"), (0, "bg")):
            assert np.array_equal(_bits(on["tensors"][k]), _bits(hb.rounded(off["tensors"][k]))), (rank, k)
            assert not np.array_equal(_bits(on["tensors"][k]), _bits(off["tensors"][k]))
        on, off = res[rank][("scatter", 1)], res[rank][("scatter", 0)]
        assert on["seen"] == off["seen"] and len(on["seen"]) == 2 and sum(on["seen"]) > 0
        assert on["stats"] == (0, 0, 2) and on["wire"] == (4, 64) and {k: on["ghosts"][k] for k in ZERO} == ZERO and on["states"] == [hg.FP32, hg.FP32]
        same(on, off, ("scatter", rank))
