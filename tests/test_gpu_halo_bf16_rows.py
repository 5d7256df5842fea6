"""dory_halo_bf16_rows (include/dorylus_hip.h): an exchange whose consumer gathers bf16 rows ships bf16 rows -- the pack rounds, 16
bits per element travel, the unpack widens into the fp32 ghost tensor -- and no bit of any result changes against the fp32 payload
under the same gather mode.  Every comparison is bit for bit; the inputs of the kernel tests are the bit patterns of
tests/halo_bf16_ref.py (ties, denormals, +-0, +-FLT_MAX, +-inf among them), which tests/test_halo_bf16_reference.py holds against torch.

  1. the kernels through dory_halo_pack / dory_halo_unpack against the numpy layout, padded and exact, every width of
     halo_exact_ref.COLS, every send count of ROWS, the ghost counts of RECV_ROWS: packed bytes, guards, statistics, raw ld-wide ghost
     rows from a buffer that ends a block of NaN into poisoned padding, dory_halo_wire_row; gather mode 1 keeps the backward pair fp32;
     dory_halo_pack_tensor keeps fp32;
  2. epochs over the in-process transport on golden partitions (P = 2, P = 3), switch on against off under the same gather mode:
     GCN (modes 1 and 2, K1s in two launches and K1, overlap on and off, exact rows 0 and 1, the transform-first order) and the GAT
     prototype (modes 1 and 2, both gat_reuse_nsum): every tensor and weight the same bits, every ghost tensor the owner's rows
     rounded where the rule says bf16 and unrounded where it says fp32, the statistics what the rule predicts;
  3. inert cases: gather mode 0, the multi-head GAT, a plan made with halo_direct_recv = 1 (the scatter transport: with 4.); the
     fused halo pack beside it;
  4. the host transport in two processes: counts and offsets in floats (rows x row_elems / 2), the switch-off bits; the scatter
     transport keeps its messages;
  5. ranks that disagree on the switch or on the gather mode fail at once with DORY_ERR_COMM and go on once fixed; refused arguments."""
import os
import sys
import time
import traceback

import numpy as np
import pytest

import halo_bf16_ref as hb
import halo_exact_ref as hx
from test_gpu_halo_exact_rows import _bits, _free_port, _golden, _plan, _raw_rows, _split_ctx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 64          # int16 elements behind a packed buffer
GUARD_VALUE = 0x5A5A


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _u16(t):
    return t.cpu().numpy().view(np.uint16)


GHOSTS = ("fg", "fgxw", "bg", "bgg", "fg_z", "bg_d")


def _same_bits(a, b, what, ghosts_too=False):
    """every downloaded local tensor, weight and gradient bit for bit; the ghost tensors (which hold rounded rows after a bf16
    exchange: _check_ghosts) only where no exchange ships bf16"""
    for r in range(len(a["tensors"])):
        assert set(a["tensors"][r]) == set(b["tensors"][r]), (what, r)
        for k in a["tensors"][r]:
            if ghosts_too or k[1] not in GHOSTS:
                assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(len(a["weights"][r])):
            for nm in a["weights"][r][l]:
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


# ---- 1. the kernels through the split entry points ---------------------------------------------------------------------------
@pytest.mark.parametrize("cols", hx.COLS)
def test_split_entry_points_pack_and_unpack_bf16_rows(da, cols):
    import torch
    from helpers import _poison_padding
    ld = hx.pad_ld(cols)
    x = hb.local_values(hx.N_LOCAL, cols)
    x2 = hb.local_values(hx.N_LOCAL, cols, salt=1)
    for ci, n_recv in enumerate(hx.RECV_ROWS[cols]):
        ctx = _split_ctx(da, cols, n_recv)
        assert ctx.halo_bf16_rows_stats() == (0, 0, 0)
        ctx.set_option("gcn_bf16_gather", 2)
        ctx.halo_bf16_rows(1)
        ctx.upload(0, "h", x)
        ctx.upload(1, "grad", x2)
        for exact in (0, 1):
            ctx.set_option("halo_exact_rows", exact)
            re = hb.row_elems(cols, bool(exact))
            assert ctx.halo_wire_row(1, da.FORWARD) == (2, re) and ctx.halo_wire_row(1, da.BACKWARD) == (2, re)
            # -- pack: every send count (the first context of a width), rows x row_elems x 2 bytes and guards behind them
            for n_send in (hx.ROWS if ci == 0 else (3,)):
                send, _ = _plan(da, ctx, da.FORWARD, n_send, n_recv, cols)
                buf = torch.full((n_send * re + GUARD,), GUARD_VALUE, dtype=torch.int16, device="cuda")
                torch.cuda.synchronize()
                assert buf.data_ptr() % 8 == 0
                before = ctx.halo_bf16_rows_stats()
                ctx.halo_pack(1, da.FORWARD, buf.data_ptr())
                ctx.sync()
                got = _u16(buf)
                want = hb.pack(x, send, cols, bool(exact))
                assert np.array_equal(got[:n_send * re], want), (cols, exact, n_send, "packed rows")
                assert (got[n_send * re:] == GUARD_VALUE).all(), (cols, exact, n_send, "guards behind the packed rows")
                after = ctx.halo_bf16_rows_stats()
                assert (after[0] - before[0], after[1] - before[1], after[2] - before[2]) == (1, n_send * re * 2, 0), (cols, exact, n_send, before, after)
            # -- a pointer off the 8-byte grid is refused, nothing is counted
            mid = ctx.halo_bf16_rows_stats()
            with pytest.raises(da.DoryError, match="error -1.*8-byte"):
                ctx.halo_pack(1, da.FORWARD, buf.data_ptr() + 4)
            assert ctx.halo_bf16_rows_stats() == mid
            # -- dory_halo_pack_tensor: the consumer is unknown, fp32 rows as without the switch
            send, _ = _plan(da, ctx, da.FORWARD, 3, n_recv, cols)
            if exact or ld % 4 == 0:
                w = cols if exact else ld
                fbuf = torch.full((3 * w + GUARD,), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                ctx.halo_pack_tensor(0, "h", da.FORWARD, fbuf.data_ptr())
                ctx.sync()
                want32 = hx.pack(x, send, cols) if exact else hx.pack_padded(x, send, cols)
                assert np.array_equal(_bits(fbuf.cpu().numpy()[:3 * w]), _bits(want32)), (cols, exact, "pack_tensor")
                assert ctx.halo_bf16_rows_stats() == (mid[0], mid[1], mid[2] + 1)
            # -- unpack: a buffer of exactly n_recv x row_elems bf16 at the end of a block of NaN, poisoned ghost padding
            _, slots = _plan(da, ctx, da.FORWARD, 3, n_recv, cols)
            _plan(da, ctx, da.BACKWARD, 3, n_recv, cols + 1000)
            bslots = hx.recv_slots(n_recv, cols + 1000)
            wire = hb.wire_values(n_recv, cols, bool(exact))
            lead = 256
            block = torch.full((lead + n_recv * re,), 0x7FC0, dtype=torch.int16, device="cuda")      # bf16 NaN in front
            if n_recv:
                block[lead:] = torch.from_numpy(wire.view(np.int16)).cuda()
            torch.cuda.synchronize()
            ptr = block.data_ptr() + 2 * lead
            for (layer, name, direction, sl) in ((1, "fg", da.FORWARD, slots), (0, "bg", da.BACKWARD, bslots)):
                assert _poison_padding(ctx, layer, name) == (ld - cols if n_recv else 0)
                ctx.halo_unpack(1, direction, ptr)
                raw = _raw_rows(ctx, layer, name)
                want = hb.unpack(np.full((n_recv, ld), np.nan, np.float32), sl, wire, cols, bool(exact))
                assert np.array_equal(_bits(raw), _bits(want)), (cols, exact, n_recv, name, "raw ghost rows")
                assert (_bits(raw[:, cols:]) == 0).all()
        # -- gather mode 1: the backward pair of the same context packs the fp32 bytes of the switch being off
        ctx.set_option("gcn_bf16_gather", 1)
        for exact in (0, 1):
            if not exact and ld % 4:
                continue                     # (a one-column tensor has no padded fp32 form)
            ctx.set_option("halo_exact_rows", exact)
            w = cols if exact else ld
            send, _ = _plan(da, ctx, da.BACKWARD, 7, n_recv, cols + 1000)
            assert ctx.halo_wire_row(1, da.BACKWARD) == (4, w) and ctx.halo_wire_row(1, da.FORWARD) == (2, hb.row_elems(cols, bool(exact)))
            got = []
            for on in (1, 0):
                ctx.halo_bf16_rows(on)
                fbuf = torch.full((7 * w + GUARD,), -7.0, dtype=torch.float32, device="cuda")
                torch.cuda.synchronize()
                before = ctx.halo_bf16_rows_stats()
                ctx.halo_pack(1, da.BACKWARD, fbuf.data_ptr())
                ctx.sync()
                after = ctx.halo_bf16_rows_stats()
                assert after == (before[0], before[1], before[2] + on), (cols, exact, on, before, after)
                got.append(fbuf.cpu().numpy())
            ctx.halo_bf16_rows(1)
            assert np.array_equal(_bits(got[0]), _bits(got[1])), (cols, exact, "backward pair under gather mode 1")
            want32 = hx.pack(x2, send, cols) if exact else hx.pack_padded(x2, send, cols)
            assert np.array_equal(_bits(got[0][:7 * w]), _bits(want32)) and (got[0][7 * w:] == -7.0).all()
        ctx.close()


# ---- 2. epochs over the in-process transport ---------------------------------------------------------------------------------
def _keep_stats(setup, kept):
    """run_local closes its contexts: read the statistics of every rank just before that"""
    def wrapped(ctx, r, g):
        setup(ctx, r, g)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"bf16": ctx.halo_bf16_rows_stats(), "fused": ctx.halo_fused_pack_stats(),
                           "rows": int(ctx.get_option("halo_rows_packed")), "floats": int(ctx.get_option("halo_floats_packed"))}
            close()
        ctx.close = closing
    return wrapped


def _own_views(pobjs):
    """the partitions' views as copies (a view's arrays live in its partition object)"""
    keys = ("localVtxCnt", "srcGhostCnt", "dstGhostCnt", "localToGlobal", "srcGhost", "dstGhost")
    return [{k: np.array(v) for k, v in p.view().items() if k in keys} for p in pobjs]


def _gcn_run(da, case, dims, epochs, opts, on, dl, fused=False, seed=5):
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
        if fused:
            ctx.halo_fused_pack(1)
        ctx.halo_bf16_rows(on)
        if opts.get("gcn_transform_first"):
            assert all(ctx.transform_first_layer(l) for l in range(L)), "the transform-first order is not active"
    kept = {}
    out = run_local(da, pobjs, parts, dims, da.GCN, epochs, _keep_stats(setup, kept), opts, downloads=dl)
    out["views"] = _own_views(pobjs)
    return out, kept


def _check_ghosts(out, pairs, what):
    """pairs: (ghost key, owner key, ghost list name, ships bf16).  A ghost tensor holds the owner's rows: rounded to bf16 where the
    exchange shipped bf16, the owner's bits where it shipped fp32"""
    views = out["views"]
    seen = 0
    for gkey, okey, lst, bf in pairs:
        g2row = {}
        for r, g in enumerate(views):
            if g["localVtxCnt"] and okey in out["tensors"][r]:
                for i, gv in enumerate(g["localToGlobal"]):
                    g2row[int(gv)] = out["tensors"][r][okey][i]
        for r, g in enumerate(views):
            if not g["localVtxCnt"] or gkey not in out["tensors"][r] or not len(g[lst]):
                continue
            want = np.stack([g2row[int(gv)] for gv in g[lst]])
            assert np.any(want != 0), (what, r, okey, "nothing travelled")
            if bf:
                want = hb.rounded(want)
            assert np.array_equal(_bits(out["tensors"][r][gkey]), _bits(want)), (what, r, gkey, "bf16" if bf else "fp32")
            seen += 1
    assert seen > 0, what


def _ghost_rows(out, lst):
    return sum(int(len(g[lst])) for g in out["views"])


GCN_DL = [(l, nm) for l in range(2) for nm in ("ah", "z")] + [(0, "h"), (0, "aTg"), (0, "bg"), (1, "grad"), (1, "fg")]


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty"])
@pytest.mark.parametrize("mode", [1, 2])
@pytest.mark.parametrize("exact", [0, 1])
def test_local_transport_gcn_epochs_bf16_rows_same_bits(da, case, mode, exact):
    """three epochs with layers of 41 floats: K1s in two launches and K1, overlap on and off; switch on against off"""
    dims, epochs = [20, 41, 6], 3
    re = hb.row_elems(41, bool(exact))
    for variant in ({"spmm_blk_nb": 8}, {"spmm_variant": 0}):
        for overlap in (1, 0):
            opts = dict(variant, halo_overlap=overlap, halo_exact_rows=exact, gcn_bf16_gather=mode)
            what = (case, mode, exact, variant, overlap)
            on, kon = _gcn_run(da, case, dims, epochs, opts, 1, GCN_DL)
            off, koff = _gcn_run(da, case, dims, epochs, opts, 0, GCN_DL)
            _same_bits(on, off, what)
            _check_ghosts(on, [((1, "fg"), (0, "h"), "srcGhost", True), ((0, "bg"), (1, "grad"), "dstGhost", mode == 2)], what)
            _check_ghosts(off, [((1, "fg"), (0, "h"), "srcGhost", False), ((0, "bg"), (1, "grad"), "dstGhost", False)], what)
            P = len(on["views"])
            assert set(kon) == set(koff) == set(range(P))
            for r in range(P):       # one forward and one backward exchange an epoch
                assert kon[r]["bf16"][0] == epochs * (2 if mode == 2 else 1) and kon[r]["bf16"][2] == epochs * (0 if mode == 2 else 1), (what, r, kon[r])
                assert koff[r]["bf16"] == (0, 0, 0) and kon[r]["rows"] == koff[r]["rows"], (what, r, kon[r], koff[r])
            rows = _ghost_rows(on, "srcGhost") + (_ghost_rows(on, "dstGhost") if mode == 2 else 0)
            assert rows > 0 and sum(kon[r]["bf16"][1] for r in range(P)) == epochs * rows * re * 2, (what, kon)


@pytest.mark.parametrize("mode", [1, 2])
def test_local_transport_gcn_transform_first_bf16_rows_same_bits(da, mode):
    """the transform-first order of every narrowing layer: xw -> fgxw forward and g -> bgg backward travel (25 -> 6 -> 3 floats).  On
    partitions built from directed records (P = 2): the golden partitions carry symmetrised edge values, with which the library
    keeps the aggregate-first order whatever the option says"""
    dims, epochs = [33, 25, 6, 3], 3
    rng = np.random.default_rng(17)
    V, E = 240, 2600
    es, ed = rng.integers(0, V, E), rng.integers(0, V, E)
    ed[:200] = 7
    es[200:400] = 13
    pv = (rng.permutation(V) % 2).astype(np.int32)
    case = lambda: ([da.Partition.build(es.astype(np.uint32), ed.astype(np.uint32), pv, r, 2) for r in range(2)], pv)
    dl = [(l, nm) for l in range(3) for nm in ("z", "bgg")] + [(l, nm) for l in (1, 2) for nm in ("xw", "fgxw")] + [(l, nm) for l in (0, 1) for nm in ("h", "aTg")]
    for exact in (0, 1):
        opts = {"spmm_blk_nb": 8, "gcn_transform_first": 2, "halo_exact_rows": exact, "gcn_bf16_gather": mode}
        on, kon = _gcn_run(da, case, dims, epochs, opts, 1, dl)
        off, koff = _gcn_run(da, case, dims, epochs, opts, 0, dl)
        _same_bits(on, off, ("transform first", mode, exact))
        _check_ghosts(on, [((l, "fgxw"), (l, "xw"), "srcGhost", True) for l in (1, 2)], ("transform first", mode, exact))
        # g is a temporary that later stages rewrite, so the backward ghost rows are held against the fp32 payload's: the switch-off
        # run's bgg, rounded where the rule says bf16
        moved = 0
        for r in range(2):
            for l in range(3):
                want = off["tensors"][r][(l, "bgg")]
                moved += int(np.any(want != 0))
                want = hb.rounded(want) if mode == 2 else want
                assert np.array_equal(_bits(on["tensors"][r][(l, "bgg")]), _bits(want)), (mode, exact, r, l, "bgg")
        assert moved > 0
        for r in range(2):       # forward: xw of layers 1 and 2; backward: g of the layers whose A^T g needs ghost rows
            nb = kon[r]["bf16"][0] + kon[r]["bf16"][2] - 2 * epochs
            assert nb > 0 and nb % epochs == 0, (mode, exact, r, kon[r])
            assert kon[r]["bf16"][0] == 2 * epochs + (nb if mode == 2 else 0) and kon[r]["bf16"][2] == (0 if mode == 2 else nb), (mode, exact, r, kon[r])
            assert koff[r]["bf16"] == (0, 0, 0) and kon[r]["rows"] == koff[r]["rows"], (mode, exact, r, kon[r], koff[r])


def _gat_run(da, gnn, case, dims, epochs, opts, on, dl, mode=0, heads=None, seed=11):
    from local_ranks import run_local
    pobjs, parts = _golden(da, case)
    V, L = len(parts), len(dims) - 1
    rng = np.random.default_rng(seed)
    H0 = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    zw = [dims[l + 1] * (heads[l] if heads and l == L - 1 else 1) for l in range(L)]      # (multi-head: hidden widths hold all heads)
    inw = [dims[0]] + zw[:-1]
    Ws = [(rng.standard_normal((inw[l], zw[l])) / np.sqrt(inw[l])).astype(np.float32) for l in range(L)]
    As = [(rng.standard_normal((dims[l + 1], 1)) / 2).astype(np.float32) for l in range(L)]
    Al = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
    Ar = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]

    def setup(ctx, r, g):
        if g["localVtxCnt"]:
            ctx.upload(0, "h", H0[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l in range(L):
            ctx.weight_set(l, "w", Ws[l])
            if gnn == da.GAT:
                ctx.weight_set(l, "a_i", As[l])
            else:
                ctx.weight_set(l, "a_l", Al[l])
                ctx.weight_set(l, "a_r", Ar[l])
        if mode:
            ctx.gat_bf16_gather(mode)
        ctx.halo_bf16_rows(on)
    kept = {}
    out = run_local(da, pobjs, parts, dims, gnn, epochs, _keep_stats(setup, kept), opts, downloads=dl,
                    pre=(lambda c: c.gatmh_heads(heads)) if heads else None, wnames=("w", "a_l", "a_r") if heads else None)
    out["views"] = _own_views(pobjs)
    return out, kept


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty"])
@pytest.mark.parametrize("mode", [1, 2])
def test_local_transport_gat_prototype_bf16_rows_same_bits(da, case, mode):
    """the GAT prototype: z -> fg_z forward (mode >= 1), grad -> bg_d backward (mode 2), both gat_reuse_nsum settings"""
    dims, epochs, L = [20, 16, 6], 3, 2
    dl = [(l, nm) for l in range(L) for nm in ("z", "ah", "grad", "aTg", "fg_z", "bg_d", "nsum")]
    for reuse in (1, 0):
        for exact in (0, 1):
            opts = {"spmm_blk_nb": 8, "gat_reuse_nsum": reuse, "halo_exact_rows": exact}
            what = (case, mode, reuse, exact)
            on, kon = _gat_run(da, da.GAT, case, dims, epochs, opts, 1, dl, mode=mode)
            off, koff = _gat_run(da, da.GAT, case, dims, epochs, opts, 0, dl, mode=mode)
            _same_bits(on, off, what)
            pairs = [((l, "fg_z"), (l, "z"), "srcGhost", True) for l in range(L)] + [((l, "bg_d"), (l, "grad"), "dstGhost", mode == 2) for l in range(L)]
            _check_ghosts(on, pairs, what)
            P = len(on["views"])
            for r in range(P):       # a forward and a backward exchange per layer and epoch
                assert kon[r]["bf16"][0] == epochs * L * (2 if mode == 2 else 1) and kon[r]["bf16"][2] == epochs * L * (0 if mode == 2 else 1), (what, r, kon[r])
                assert koff[r]["bf16"] == (0, 0, 0)
            rows = _ghost_rows(on, "srcGhost") + (_ghost_rows(on, "dstGhost") if mode == 2 else 0)
            want = epochs * rows * 2 * sum(hb.row_elems(dims[l + 1], bool(exact)) for l in range(L))
            assert rows > 0 and sum(kon[r]["bf16"][1] for r in range(P)) == want, (what, kon)


# ---- 3. inert cases ----------------------------------------------------------------------------------------------------------
def _inert(kon, koff, epochs_exchanges, what):
    for r in kon:
        assert kon[r]["bf16"][0] == 0 and kon[r]["bf16"][1] == 0 and kon[r]["bf16"][2] == epochs_exchanges, (what, r, kon[r])
        assert koff[r]["bf16"] == (0, 0, 0) and kon[r]["rows"] == koff[r]["rows"] and kon[r]["floats"] == koff[r]["floats"], (what, r, kon[r], koff[r])


def test_gather_mode_0_keeps_fp32_rows(da):
    dims, epochs = [20, 41, 6], 2
    opts = {"spmm_blk_nb": 8, "gcn_bf16_gather": 0}
    on, kon = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 1, GCN_DL)
    off, koff = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 0, GCN_DL)
    _same_bits(on, off, "gather mode 0", ghosts_too=True)
    _check_ghosts(on, [((1, "fg"), (0, "h"), "srcGhost", False), ((0, "bg"), (1, "grad"), "dstGhost", False)], "gather mode 0")
    _inert(kon, koff, 2 * epochs, "gather mode 0")


def test_plan_made_with_halo_direct_recv_keeps_fp32_rows(da):
    dims, epochs = [20, 41, 6], 2
    for exact in (0, 1):
        opts = {"spmm_blk_nb": 8, "gcn_bf16_gather": 2, "halo_direct_recv": 1, "halo_exact_rows": exact}
        on, kon = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 1, GCN_DL)
        off, koff = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 0, GCN_DL)
        _same_bits(on, off, ("halo_direct_recv", exact), ghosts_too=True)
        _check_ghosts(on, [((1, "fg"), (0, "h"), "srcGhost", False), ((0, "bg"), (1, "grad"), "dstGhost", False)], ("halo_direct_recv", exact))
        _inert(kon, koff, 2 * epochs, ("halo_direct_recv", exact))


def test_multi_head_gat_keeps_fp32_rows(da):
    """one epoch of the 8-head extension on a golden partition, P = 2: never bf16 on the wire"""
    dims, heads = [20, 128, 6], [8, 1]
    dl = [(l, nm) for l in range(2) for nm in ("z", "o", "dz", "fg_z", "bg_do", "bg_st")] + [(1, "logits")]
    opts = {"spmm_blk_nb": 8}
    on, kon = _gat_run(da, da.GATMH, "parts_toy60_p2", dims, 1, opts, 1, dl, heads=heads)
    off, koff = _gat_run(da, da.GATMH, "parts_toy60_p2", dims, 1, opts, 0, dl, heads=heads)
    _same_bits(on, off, "8-head GAT", ghosts_too=True)
    _check_ghosts(on, [((l, "fg_z"), (l, "z"), "srcGhost", False) for l in range(2)], "8-head GAT")
    for r in kon:
        assert kon[r]["bf16"][:2] == (0, 0) and kon[r]["bf16"][2] > 0 and koff[r]["bf16"] == (0, 0, 0), (r, kon[r])
        assert kon[r]["rows"] == koff[r]["rows"] and kon[r]["floats"] == koff[r]["floats"]


def test_fused_halo_pack_beside_bf16_rows(da):
    """with dory_halo_fused_pack on too: the exchanges that ship bf16 run the pack kernel and count as its fallbacks, the fp32 ones
    still fuse, and the bits stay equal"""
    dims, epochs = [20, 41, 6], 3
    for mode, exact in ((2, 0), (1, 1)):
        opts = {"spmm_blk_nb": 8, "gcn_bf16_gather": mode, "halo_exact_rows": exact}
        plain, _ = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 0, GCN_DL)
        fo, kfo = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 0, GCN_DL, fused=True)
        fb, kfb = _gcn_run(da, "parts_toy60_p2", dims, epochs, opts, 1, GCN_DL, fused=True)
        _same_bits(fb, plain, ("fused + bf16 against neither", mode))
        _same_bits(fo, plain, ("fused against neither", mode), ghosts_too=True)
        for r in range(2):
            assert kfo[r]["fused"][0] == 2 * epochs and kfo[r]["fused"][2] == 0, (mode, r, kfo[r])      # h and grad both come out of GEMMs
            nbf = epochs * (2 if mode == 2 else 1)
            assert kfb[r]["bf16"][0] == nbf and kfb[r]["fused"][0] == 2 * epochs - nbf and kfb[r]["fused"][2] == nbf, (mode, r, kfb[r])
            assert kfb[r]["bf16"][2] == 2 * epochs - nbf


# ---- 4. the host transport and the scatter transport, two processes -----------------------------------------------------------
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

        def run(transport, exact, on):
            ctx = da.Context(0)
            ctx.configure(da.GCN, dims, V, rank, world)
            for k, v in (("spmm_blk_nb", 8), ("halo_exact_rows", exact), ("gcn_bf16_gather", 2)):
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
            ctx.halo_bf16_rows(on)
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
            res = {"seen": seen, "stats": ctx.halo_bf16_rows_stats(), "wire": ctx.halo_wire_row(1, da.FORWARD), "tensors": {}, "W": [], "dW": []}
            for l, nm in ((0, "ah"), (1, "ah"), (0, "h"), (0, "aTg"), (1, "grad"), (1, "fg"), (0, "bg")):
                if ctx.info(l, nm)[0]:
                    res["tensors"][(l, nm)] = ctx.download(l, nm)
            for l in range(L):
                res["W"].append(ctx.weight_get(l))
                res["dW"].append(ctx.weight_grad_get(l))
            eng.close()
            ctx.close()
            return res
        out = {(t, e, on): run(t, e, on) for t, e in (("host", 0), ("host", 1), ("scatter", 0)) for on in (1, 0)}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_host_transport_counts_in_floats_and_scatter_transport_inert():
    """two processes on one GPU, the bytes over gloo.  Host transport: the counts and offsets the callback is given are
    rows x row_elems / 2 floats (rows x 32 for the padded 64, rows x 22 for the exact 44), the epoch's bits are the switch-off
    bits and the ghost rows arrive rounded.  Scatter transport: the same message bytes with the switch on, no bf16 pack."""
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
        for exact, per_row_on, per_row_off in ((0, 32, 64), (1, 22, 41)):
            on, off = res[rank][("host", exact, 1)], res[rank][("host", exact, 0)]
            assert len(on["seen"]) == len(off["seen"]) == 2
            for c_on, c_off in zip(on["seen"], off["seen"]):
                for a_on, a_off in zip(c_on, c_off):
                    assert all(x % per_row_off == 0 for x in a_off), (rank, a_off)
                    assert a_on == [x // per_row_off * per_row_on for x in a_off], (rank, exact, a_on, a_off)
            assert sum(sum(c[0]) + sum(c[2]) for c in on["seen"]) > 0
            rows = sum(sum(c[0]) for c in off["seen"]) // per_row_off
            assert on["stats"] == (2, rows * per_row_on * 4, 0) and off["stats"] == (0, 0, 0), (rank, exact, on["stats"])
            assert on["wire"] == (2, 2 * per_row_on) and off["wire"] == (4, per_row_off)
            same(on, off, ("host", rank, exact), skip=((1, "fg"), (0, "bg")))       # the ghost tensors hold rounded rows
            for k in ((1, "fg"), (0, "bg")):
                if k in on["tensors"]:
                    assert np.array_equal(_bits(on["tensors"][k]), _bits(hb.rounded(off["tensors"][k]))), (rank, exact, k)
        on, off = res[rank][("scatter", 0, 1)], res[rank][("scatter", 0, 0)]
        assert on["seen"] == off["seen"] and len(on["seen"]) == 2 and sum(on["seen"]) > 0
        assert on["stats"] == (0, 0, 2) and off["stats"] == (0, 0, 0) and on["wire"] == (4, 64)
        same(on, off, ("scatter", rank))
    for exact in (0, 1):       # rank 0's send counts are rank 1's receive counts
        for c0, c1 in zip(res[0][("host", exact, 1)]["seen"], res[1][("host", exact, 1)]["seen"]):
            assert c0[0][1] == c1[2][0] and c1[0][0] == c0[2][1]


# ---- 5. ranks that disagree, refused arguments -------------------------------------------------------------------------------
def test_local_transport_refuses_ranks_that_disagree_at_once(da):
    """rank 0 with the switch on, rank 1 off (both gather mode 2): the exchange fails with DORY_ERR_COMM on either rank before
    anything is enqueued or counted, well inside local_timeout_ms; fixed, the exchange runs and the ghost rows are the owners'
    rounded.  Then the switch on everywhere and the gather mode 2 on rank 0, 0 on rank 1: the same, and on again once fixed"""
    pobjs, parts = _golden(da, "parts_toy60_p2")
    gs = [p.view() for p in pobjs]
    rng = np.random.default_rng(3)
    ctxs, H = [], []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GCN, [20, 41, 6], len(parts), r, 2)
        for k, v in (("spmm_blk_nb", 8), ("local_timeout_ms", 2000), ("gcn_bf16_gather", 2)):
            ctx.set_option(k, v)
        part.upload(ctx, parts)
        ctx.preallocate()
        ctx.halo_bf16_rows(1 - r)
        H.append(rng.uniform(-1, 1, (int(gs[r]["localVtxCnt"]), 41)).astype(np.float32))
        ctx.upload(0, "h", H[r])
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    g2row = {int(gv): H[r][i] for r in (0, 1) for i, gv in enumerate(gs[r]["localToGlobal"])}

    def refused():
        for r in (0, 1):
            before = ctxs[r].halo_bf16_rows_stats(), int(ctxs[r].get_option("halo_rows_packed"))
            t0 = time.perf_counter()
            with pytest.raises(da.DoryError, match=r"error -4.*dory_halo_bf16_rows differs.*rank %d ships %s rows, rank %d %s rows"
                               % (r, "bf16" if r == 0 else "fp32", 1 - r, "fp32" if r == 0 else "bf16")):
                ctxs[r].halo_exchange(1, da.FORWARD)
            assert time.perf_counter() - t0 < 1.0
            assert (ctxs[r].halo_bf16_rows_stats(), int(ctxs[r].get_option("halo_rows_packed"))) == before

    def runs(n_before):
        ctxs[0].halo_exchange(1, da.FORWARD)            # first half
        ctxs[1].halo_exchange(1, da.FORWARD)
        ctxs[0].sync()
        ctxs[1].sync()
        for r in (0, 1):
            if gs[r]["srcGhostCnt"]:
                want = hb.rounded(np.stack([g2row[int(gv)] for gv in gs[r]["srcGhost"]]))
                assert np.array_equal(_bits(ctxs[r].download(1, "fg")), _bits(want)), r
            assert ctxs[r].halo_bf16_rows_stats()[0] == n_before + 1
    refused()
    ctxs[1].halo_bf16_rows(1)
    runs(0)
    ctxs[1].set_option("gcn_bf16_gather", 0)
    refused()
    ctxs[1].set_option("gcn_bf16_gather", 2)
    runs(1)
    for c in ctxs:
        c.close()


def test_refused_arguments_and_single_partition(da):
    import aggregate_ref as ar
    from helpers import make_ctx
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="error -1.*halo_bf16_rows"):
        c.halo_bf16_rows(1)                          # before dory_configure
    c.close()
    ctx = _split_ctx(da, 41, 3)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="error -1.*halo_bf16_rows"):
            ctx.halo_bf16_rows(bad)
    assert ctx.halo_wire_row(1, da.FORWARD) == (4, 64)
    with pytest.raises(da.DoryError, match="error -1.*halo_wire_row"):
        ctx.halo_wire_row(0, da.FORWARD)
    with pytest.raises(da.DoryError, match="error -1.*halo_wire_row"):
        ctx.halo_wire_row(1, 2)
    ctx.close()
    # a single partition: accepted and inert; refused while an epoch graph is being recorded
    one = make_ctx(da, ar.graph("uniform:64:300"), [4, 41, 2], 64, options={"gcn_bf16_gather": 2})
    one.halo_bf16_rows(1)
    one.halo_exchange(1, da.FORWARD)
    one.sync()
    assert one.halo_bf16_rows_stats() == (0, 0, 0)
    one.epoch_graph_begin()
    with pytest.raises(da.DoryError, match="error -1.*epoch graph is being recorded"):
        one.halo_bf16_rows(0)
    one.epoch_graph_drop()
    one.halo_bf16_rows(0)
    one.close()
