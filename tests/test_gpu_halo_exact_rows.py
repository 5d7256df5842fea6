"""Option halo_exact_rows (include/dorylus_hip.h): packed halo rows hold exactly `cols` floats instead of the padded `ld`, in
every transport and in the split entry points, and no bit of any result changes.

  1. the kernels through dory_halo_pack / dory_halo_unpack (and the *_tensor forms on other tensors) against the numpy layout
     (tests/halo_exact_ref.py): a send buffer of exactly n x cols floats with guards behind it, a receive buffer that is the
     end of a block of NaN, poisoned ghost padding, the raw ld-wide ghost rows bit-equal to the padded form's, the counters;
  2. whole epochs over the in-process device transport, option 1 against option 0 bit for bit and against the oracle, as
     tests/test_gpu_local_transport.py checks them (its helpers are copied here): GCN on the golden partitions with K1s in
     two launches and K1, overlap on and off, the transform-first order, the GAT prototype, the 8-head GAT (do / st exchange);
  3. ranks that disagree on the option fail at once with DORY_ERR_COMM, and go on after the option is fixed;
  4. the host transport: the counts and offsets the callback is given are rows x cols, one epoch gives option 0's bits.
Not covered: the refusal of a source / ghost pair whose `cols` differ.  dory_preallocate lays both tensors of every pair out from
the same entry of dims, so no sequence of public calls builds such a pair; the check (DORY_ERR_ARG in exchange_rows,
dory_halo_pack, dory_halo_unpack) guards future tensor tables.  The misaligned pointer is covered.
Reference: Engine::verticesPushOut ships featDim floats per row (engine/utils.cpp:623-650)."""
import ctypes as C
import glob
import os
import socket
import sys
import time
import traceback

import numpy as np
import pytest

import halo_exact_ref as hx

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4
COUNTERS = ("halo_rows_packed", "halo_floats_packed", "halo_exact_packs")


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _counters(ctx):
    return tuple(int(ctx.get_option(k)) for k in COUNTERS)


# ---- 1. the kernels through the split entry points ---------------------------------------------------------------------------
def _raw_rows(ctx, layer, name):
    """the raw ld-wide rows of a device tensor, through its dory_tensor_info pointer"""
    rows, cols, ld, p = ctx.info(layer, name)
    out = np.empty((rows, ld), np.float32)
    if rows == 0:
        return out
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    ctx.sync()
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) == 0
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _split_ctx(da, cols, n_recv):
    """rank 0 of 2 on a partition with n_recv ghost rows on both sides; GCN dims [4, cols, 2]: h@0 -> fg@1 forward,
    grad@1 -> bg@0 backward, both `cols` wide"""
    import aggregate_ref as ar
    from helpers import make_ctx
    g = ar.graph(hx.graph_name(n_recv))
    return make_ctx(da, g, [4, cols, 2], int(g["globalVtxCnt"]) + 1, node_id=0, num_nodes=2)


def _plan(da, ctx, direction, n_send, n_recv, seed):
    send, slots = hx.send_list(n_send, seed), hx.recv_slots(n_recv, seed)
    ctx.halo_plan(direction, [[], send], [[], slots])
    return send, slots


@pytest.mark.parametrize("cols", hx.COLS)
def test_split_entry_points_pack_and_unpack_exact_rows(da, cols):
    import torch
    from helpers import _poison_padding
    ld = hx.pad_ld(cols)
    GUARD = 64
    for n_recv in hx.RECV_ROWS[cols]:
        ctx = _split_ctx(da, cols, n_recv)
        assert ctx.get_option("halo_exact_rows") == 0 and _counters(ctx) == (0, 0, 0)
        ctx.set_option("halo_exact_rows", 1)
        x = hx.local_values(cols)
        ctx.upload(0, "h", x)
        x2 = hx.local_values(cols, salt=1)
        ctx.upload(0, "z", x2)
        # -- pack: every send count of the list, exactly n x cols floats and guards behind them
        for n_send in hx.ROWS:
            send, slots = _plan(da, ctx, da.FORWARD, n_send, n_recv, cols)
            buf = torch.full((n_send * cols + GUARD,), -7.0, dtype=torch.float32, device="cuda")
            torch.cuda.synchronize()     # (torch's fill runs on torch's stream, the pack on the context's non-blocking one)
            assert buf.data_ptr() % 16 == 0
            before = _counters(ctx)
            ctx.halo_pack(1, da.FORWARD, buf.data_ptr())
            ctx.sync()
            got = buf.cpu().numpy()
            want = hx.pack(x, send, cols)
            assert np.array_equal(_bits(got[:n_send * cols]), _bits(want)), (cols, n_send, "packed rows")
            assert (got[n_send * cols:] == -7.0).all(), (cols, n_send, "guards behind the packed rows")
            after = _counters(ctx)
            assert after[0] - before[0] == n_send and after[1] - before[1] == n_send * cols, (cols, n_send, before, after)
            assert after[2] - before[2] == (1 if cols < ld else 0), (cols, n_send, before, after)
            # the *_tensor form on another tensor
            buf.fill_(-7.0)
            torch.cuda.synchronize()
            ctx.halo_pack_tensor(0, "z", da.FORWARD, buf.data_ptr())
            ctx.sync()
            got = buf.cpu().numpy()
            assert np.array_equal(_bits(got[:n_send * cols]), _bits(hx.pack(x2, send, cols))), (cols, n_send, "pack_tensor")
            assert (got[n_send * cols:] == -7.0).all(), (cols, n_send, "pack_tensor guards")
            if n_send and cols % 4:      # a pointer off the 16-byte grid is refused, nothing is written or counted
                mid = _counters(ctx)
                with pytest.raises(da.DoryError, match="error -1.*16-byte"):
                    ctx.halo_pack(1, da.FORWARD, buf.data_ptr() + 4)
                with pytest.raises(da.DoryError, match="error -1.*16-byte"):
                    ctx.halo_pack_tensor(0, "z", da.FORWARD, buf.data_ptr() + 8)
                assert _counters(ctx) == mid
        # -- unpack: a buffer of exactly n_recv x cols floats at the end of a block of NaN, poisoned ghost padding
        send, slots = _plan(da, ctx, da.FORWARD, 3, n_recv, cols)
        _plan(da, ctx, da.BACKWARD, 3, n_recv, cols + 1000)
        _, bslots = hx.send_list(3, cols + 1000), hx.recv_slots(n_recv, cols + 1000)
        wire = hx.wire_values(n_recv, cols)
        lead = 256                                        # floats of NaN in front: the buffer starts on a 16-byte boundary
        block = torch.full((lead + n_recv * cols,), float("nan"), dtype=torch.float32, device="cuda")
        block[lead:] = torch.from_numpy(wire).cuda()
        ptr = block.data_ptr() + 4 * lead
        torch.cuda.synchronize()
        for (layer, name, direction, sl, by_name) in ((1, "fg", da.FORWARD, slots, False), (0, "bg", da.BACKWARD, bslots, True)):
            assert _poison_padding(ctx, layer, name) == (ld - cols if n_recv else 0)
            if by_name:
                ctx.halo_unpack_tensor(layer, name, direction, ptr)
            else:
                ctx.halo_unpack(layer, direction, ptr)
            raw = _raw_rows(ctx, layer, name)
            assert not np.isnan(raw).any(), (cols, n_recv, name, "NaN arrived")
            want = hx.unpack(np.full((n_recv, ld), np.nan, np.float32), sl, wire, cols)
            assert np.array_equal(_bits(raw), _bits(want)), (cols, n_recv, name, "raw ghost rows")
            if n_recv and cols % 4:
                with pytest.raises(da.DoryError, match="error -1.*16-byte"):
                    (ctx.halo_unpack_tensor(layer, name, direction, ptr + 4) if by_name else ctx.halo_unpack(layer, direction, ptr + 4))
            if ld % 4 == 0:      # and the padded form's raw rows from the padded buffer of the same rows: the same bits
                ctx.set_option("halo_exact_rows", 0)
                padded = np.zeros((n_recv, ld), np.float32)
                padded[:, :cols] = wire.reshape(n_recv, cols)
                pbuf = torch.from_numpy(padded.reshape(-1)).cuda() if n_recv else torch.zeros(4, device="cuda")
                _poison_padding(ctx, layer, name)
                torch.cuda.synchronize()
                if by_name:
                    ctx.halo_unpack_tensor(layer, name, direction, pbuf.data_ptr())
                else:
                    ctx.halo_unpack(layer, direction, pbuf.data_ptr())
                raw0 = _raw_rows(ctx, layer, name)
                assert np.array_equal(_bits(raw), _bits(raw0)), (cols, n_recv, name, "exact against padded unpack")
                ctx.set_option("halo_exact_rows", 1)
        assert ctx.download(1, "fg").shape == (n_recv, cols)
        ctx.close()


def test_option_values_and_padded_default(da):
    """values outside {0, 1} are refused on every model; with 0 the packs count padded rows and no exact pack; a single
    partition keeps exchanging nothing"""
    import torch
    ctx = _split_ctx(da, 41, 3)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="halo_exact_rows"):
            ctx.set_option("halo_exact_rows", bad)
    assert ctx.get_option("halo_exact_rows") == 0
    for k in COUNTERS:
        with pytest.raises(da.DoryError):
            ctx.set_option(k, 1)
    send, _ = _plan(da, ctx, da.FORWARD, 7, 3, 1)
    x = hx.local_values(41)
    ctx.upload(0, "h", x)
    buf = torch.zeros(7 * 64, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.halo_pack(1, da.FORWARD, buf.data_ptr())
    ctx.sync()
    assert np.array_equal(buf.cpu().numpy(), hx.pack_padded(x, send, 41))
    assert _counters(ctx) == (7, 7 * 64, 0)
    ctx.close()
    for gnn in (da.GAT, da.GATMH):
        c = da.Context(0)
        c.set_option("halo_exact_rows", 1)
        c.configure(gnn, [8, 16, 4], 10)
        assert c.get_option("halo_exact_rows") == 1
        c.close()
    import aggregate_ref as ar
    from helpers import make_ctx
    one = make_ctx(da, ar.graph("uniform:64:300"), [4, 41, 2], 64, options={"halo_exact_rows": 1})
    one.halo_exchange(1, da.FORWARD)
    one.sync()
    assert _counters(one) == (0, 0, 0)
    one.close()


# ---- 2. the in-process device transport (helpers of tests/test_gpu_local_transport.py, copied) -------------------------------
def _golden(da, name):
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


def _keep_counters(setup, kept):
    """run_local closes its contexts: read the halo counters of every rank just before that"""
    def wrapped(ctx, r, g):
        setup(ctx, r, g)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = _counters(ctx)
            close()
        ctx.close = closing
    return wrapped


def _gcn_case(da, pobjs, parts, dims, epochs, opts, seed=5, kept=None):
    from local_ranks import run_local
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
    dl = [(l, nm) for l in range(L) for nm in ("ah",)] + [(l, nm) for l in range(L - 1) for nm in ("h", "aTg", "bg")] + \
         [(l, nm) for l in range(1, L) for nm in ("grad", "fg")]
    out = run_local(da, pobjs, parts, dims, da.GCN, epochs, setup if kept is None else _keep_counters(setup, kept), opts, downloads=dl)
    return out, (X, labels, Ws)


def _oracle_epochs(gs, parts, X, labels, Ws, epochs):
    import orc
    from helpers import oracle_gcn_epoch
    V, L = len(parts), len(Ws)
    Wo = [w.copy() for w in Ws]
    m = [np.zeros_like(w) for w in Ws]
    v = [np.zeros_like(w) for w in Ws]
    T = dW = None
    for ep in range(epochs):
        T, dW = oracle_gcn_epoch(gs, parts, X, labels, Wo, V)
        for l in range(L - 1, -1, -1):
            orc.adam_update(Wo[l], dW[l], m[l], v[l], 0.01, ep + 1)
    return T, dW, Wo


def _check_vs_oracle(out, gs, T, dW, Wo, L, what):
    from helpers import assert_parity, rel_err
    for r, g in enumerate(gs):
        t = out["tensors"][r]
        if not g["localVtxCnt"]:
            continue
        for l in range(L):
            assert_parity(t[(l, "ah")], T[r][f"ah{l}"], (what, r, l, "ah"))
            if l < L - 1:
                assert_parity(t[(l, "h")], T[r][f"h{l}"], (what, r, l, "h"))
                assert_parity(t[(l, "aTg")], T[r][f"aTg{l}"], (what, r, l, "aTg"))
            if l > 0:
                assert rel_err(t[(l, "grad")], T[r][f"grad{l}"]) < RTOL, (what, r, l, "grad")
                if g["srcGhostCnt"]:
                    assert_parity(t[(l, "fg")], T[r][f"fg{l}"], (what, r, l, "fg"))
                if g["dstGhostCnt"]:
                    assert rel_err(t[(l - 1, "bg")], T[r][f"bg{l-1}"]) < RTOL, (what, r, l, "bg")
        for l in range(L):
            assert rel_err(out["wgrads"][r][l]["w"], dW[l]) < RTOL, (what, r, "dW", l)       # the summed gradient, on every rank
            assert rel_err(out["weights"][r][l]["w"], Wo[l]) < RTOL, (what, r, "W", l)
    # ghost rows are the owners' rows bit for bit; the gradient sum and the weights are the same bits on every rank
    for l in range(1, L):
        g2row = {}
        for r, g in enumerate(gs):
            if g["localVtxCnt"]:
                for i, gv in enumerate(g["localToGlobal"]):
                    g2row[int(gv)] = (out["tensors"][r][(l - 1, "h")][i], out["tensors"][r][(l, "grad")][i])
        for r, g in enumerate(gs):
            if g["localVtxCnt"] and g["srcGhostCnt"]:
                assert np.array_equal(out["tensors"][r][(l, "fg")], np.stack([g2row[int(gv)][0] for gv in g["srcGhost"]])), (what, r, l, "fg bits")
            if g["localVtxCnt"] and g["dstGhostCnt"]:
                assert np.array_equal(out["tensors"][r][(l - 1, "bg")], np.stack([g2row[int(gv)][1] for gv in g["dstGhost"]])), (what, r, l, "bg bits")
    # the validation statistics summed over the partitions (dory_train_stat_global = the weight servers' updateGlobalAccLoss):
    # the sum of the ranks' own, the same on every rank, and the oracle's
    loc = [s[0] for s in out["stats"]]
    for r, (mine, glob) in enumerate(out["stats"]):
        assert glob[2] == sum(x[2] for x in loc) and glob == out["stats"][0][1], (what, r, glob)
        assert abs(glob[0] - sum(x[0] for x in loc)) < 1e-3 and abs(glob[1] - sum(x[1] for x in loc)) <= 1e-5 * max(1.0, abs(glob[1])), (what, r, glob, loc)
    assert abs(out["stats"][0][1][1] - sum(T[r].get("loss", 0.0) for r in range(len(gs)))) <= 1e-4 * max(1.0, abs(out["stats"][0][1][1])), what
    for r in range(1, len(gs)):
        for l in range(L):
            assert np.array_equal(out["wgrads"][r][l]["w"], out["wgrads"][0][l]["w"]), (what, r, l, "dW bits")
            assert np.array_equal(out["weights"][r][l]["w"], out["weights"][0][l]["w"]), (what, r, l, "W bits")


def _same_bits(a, b, what):
    for r in range(len(a["tensors"])):
        assert set(a["tensors"][r]) == set(b["tensors"][r]), (what, r)
        for k in a["tensors"][r]:
            assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(len(a["weights"][r])):
            for nm in a["weights"][r][l]:
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


def _gcn_exact_against_padded(da, case, dims, epochs, variants, overlaps, oracle=True, extra=None):
    for opts in variants:
        for overlap in overlaps:
            runs, kept = [], []
            for exact in (1, 0):
                pobjs, parts = _golden(da, case)
                gs = [p.view() for p in pobjs]
                k = {}
                out, (X, labels, Ws) = _gcn_case(da, pobjs, parts, dims, epochs,
                                                 dict(opts, halo_overlap=overlap, halo_exact_rows=exact, **(extra or {})), kept=k)
                if oracle:
                    T, dW, Wo = _oracle_epochs(gs, parts, X, labels, Ws, epochs)
                    _check_vs_oracle(out, gs, T, dW, Wo, len(dims) - 1, (case, opts, overlap, exact))
                runs.append(out)
                kept.append(k)
            _same_bits(runs[0], runs[1], (case, dims, opts, overlap, "halo_exact_rows 1 / 0"))
            yield kept, len(runs[0]["tensors"])


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy97_p8_und", "parts_toy60_p4_hash", "parts_toy40_p3_empty"])
def test_local_transport_gcn_epochs_exact_rows_same_bits(da, case):
    """three epochs with layers of 41 floats (64 padded), K1s in two launches and the row gather, overlap on and off: every
    downloaded tensor, weight and gradient the same bits with the option 1 and 0, ghost rows the owners' bits, the oracle's
    epochs by the existing criteria; what the packs wrote is rows x 41 floats against rows x 64"""
    dims, epochs = [20, 41, 6], 3
    for kept, P in _gcn_exact_against_padded(da, case, dims, epochs, ({"spmm_blk_nb": 8}, {"spmm_variant": 0}), (1, 0)):
        k1, k0 = kept
        assert set(k1) == set(k0) == set(range(P))
        for r in range(P):
            assert k1[r][0] == k0[r][0], (case, r, k1, k0)                               # the same rows travelled
            assert k1[r][1] == k1[r][0] * 41 and k0[r][1] == k0[r][0] * 64, (case, r, k1[r], k0[r])
            assert k0[r][2] == 0
        assert sum(k1[r][0] for r in range(P)) > 0 and sum(k1[r][2] for r in range(P)) > 0, (case, k1)


def test_local_transport_gcn_three_layers_odd_widths(da):
    """layers of 25, 6 and 3 floats (rows of 25 -> 32 and 6 -> 32 travel; quads straddle rows in both)"""
    for kept, P in _gcn_exact_against_padded(da, "parts_toy60_p4_hash", [33, 25, 6, 3], 3, ({"spmm_blk_nb": 8}, {"spmm_variant": 0}), (1, 0)):
        k1, k0 = kept
        for r in range(P):
            assert k1[r][0] == k0[r][0] and k1[r][1] < k0[r][1] or k1[r][0] == 0, (r, k1[r], k0[r])


def test_local_transport_gcn_transform_first_exact_rows_same_bits(da):
    """the transform-first order of every narrowing layer (xw / g travel): the same bits with the option 1 and 0"""
    for kept, P in _gcn_exact_against_padded(da, "parts_toy60_p2", [33, 25, 6, 3], 3, ({"spmm_blk_nb": 8},), (1, 0), oracle=False,
                                             extra={"gcn_transform_first": 2}):
        k1, k0 = kept
        assert all(k1[r][0] == k0[r][0] for r in range(P))


def test_local_transport_gat_prototype_exact_rows_same_bits(da):
    """the GAT prototype: z (16 of 32 floats: the existing kernels at the exact width; 6 of 32: the new ones) forward, grad
    backward"""
    from local_ranks import run_local
    case, dims, L = "parts_toy60_p2", [20, 16, 6], 2
    for overlap in (1, 0):
        runs, kept = [], []
        for exact in (1, 0):
            pobjs, parts = _golden(da, case)
            V = len(parts)
            rng = np.random.default_rng(11)
            H0 = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
            labels = rng.integers(0, dims[-1], V).astype(np.uint32)
            Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]
            As = [(rng.standard_normal((dims[i + 1], 1)) / 2).astype(np.float32) for i in range(L)]

            def setup(ctx, r, g):
                if g["localVtxCnt"]:
                    ctx.upload(0, "h", H0[g["localToGlobal"]])
                ctx.labels_upload(labels[g["localToGlobal"]])
                for l in range(L):
                    ctx.weight_set(l, "w", Ws[l])
                    ctx.weight_set(l, "a_i", As[l])
            dl = [(l, nm) for l in range(L) for nm in ("z", "ah", "grad", "aTg", "fg_z", "bg_d")]
            k = {}
            runs.append(run_local(da, pobjs, parts, dims, da.GAT, 3, _keep_counters(setup, k),
                                  {"spmm_blk_nb": 8, "halo_overlap": overlap, "halo_exact_rows": exact}, downloads=dl))
            kept.append(k)
        _same_bits(runs[0], runs[1], ("GAT prototype", overlap, "halo_exact_rows 1 / 0"))
        for r in range(2):
            assert kept[0][r][0] == kept[1][r][0] > 0 and kept[0][r][1] < kept[1][r][1] and kept[0][r][2] > 0 == kept[1][r][2], kept


def test_local_transport_gat_mh_exact_rows_same_bits(da):
    """the 8-head extension at P = 2: z forward, and do / st between the two phases of the backward sweep, through the same
    exchange_rows (rows of 128 = ld, 41 of 64, 32 = ld and 4 of 32 floats)"""
    from local_ranks import run_local
    P, dims, heads, V, E = 2, [40, 128, 41], [8, 1], 240, 2600
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % P).astype(np.int32)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = []
    for l in range(2):
        zw = dims[l + 1] * (heads[l] if l == 1 else 1)
        params.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                       (rng.standard_normal(zw) * 0.3).astype(np.float32), (rng.standard_normal(zw) * 0.3).astype(np.float32)])

    def setup(ctx, r, g):
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W)
            ctx.weight_set(l, "a_l", al)
            ctx.weight_set(l, "a_r", ar)
    dl = [(l, nm) for l in range(2) for nm in ("z", "o", "t", "del", "der", "dz", "fg_z", "bg_do", "bg_st")] + [(1, "logits")]
    runs, kept = [], []
    for exact in (1, 0):
        pobjs = [da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, P) for r in range(P)]
        k = {}
        runs.append(run_local(da, pobjs, parts, dims, da.GATMH, 2, _keep_counters(setup, k), {"spmm_blk_nb": 8, "halo_exact_rows": exact},
                              downloads=dl, pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r")))
        kept.append(k)
    _same_bits(runs[0], runs[1], ("8-head GAT", "halo_exact_rows 1 / 0"))
    for r in range(P):
        assert kept[0][r][0] == kept[1][r][0] > 0 and kept[0][r][1] < kept[1][r][1] and kept[0][r][2] > 0 == kept[1][r][2], kept


# ---- 3. ranks that disagree ------------------------------------------------------------------------------------------------
def test_local_transport_refuses_ranks_that_disagree_at_once(da):
    """rank 0 with the option 1, rank 1 with 0: the exchange fails with DORY_ERR_COMM naming both ranks before anything is
    enqueued or counted -- well inside local_timeout_ms -- on either rank; after the option is fixed the next exchange runs"""
    pobjs, parts = _golden(da, "parts_toy60_p2")
    gs = [p.view() for p in pobjs]
    rng = np.random.default_rng(3)
    ctxs, H = [], []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GCN, [20, 41, 6], len(parts), r, 2)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("local_timeout_ms", 2000)
        ctx.set_option("halo_exact_rows", 1 - r)
        part.upload(ctx, parts)
        ctx.preallocate()
        H.append(rng.uniform(-1, 1, (int(gs[r]["localVtxCnt"]), 41)).astype(np.float32))
        ctx.upload(0, "h", H[r])
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    for r in (0, 1):
        t0 = time.perf_counter()
        with pytest.raises(da.DoryError, match=r"error -4.*halo_exact_rows.*rank %d has %d.*rank %d has %d" % (r, 1 - r, 1 - r, r)):
            ctxs[r].halo_exchange(1, da.FORWARD)
        assert time.perf_counter() - t0 < 1.0
        assert _counters(ctxs[r]) == (0, 0, 0)
    ctxs[1].set_option("halo_exact_rows", 1)
    ctxs[0].halo_exchange(1, da.FORWARD)            # first half
    ctxs[1].halo_exchange(1, da.FORWARD)
    ctxs[0].sync()
    ctxs[1].sync()
    g2row = {int(gv): H[r][i] for r in (0, 1) for i, gv in enumerate(gs[r]["localToGlobal"])}
    for r in (0, 1):
        if gs[r]["srcGhostCnt"]:
            want = np.stack([g2row[int(gv)] for gv in gs[r]["srcGhost"]])
            assert np.array_equal(_bits(ctxs[r].download(1, "fg")), _bits(want)), r
        rows, floats, ex = _counters(ctxs[r])
        assert floats == rows * 41 and ex == 1
    for c in ctxs:
        c.close()


# ---- 4. the host transport (worker pattern of tests/test_gpu_multirank.py, copied) -----------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, exact, q):
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
        gs = [p.view() for p in pobjs]
        part, g = pobjs[rank], gs[rank]
        V, L = len(parts), len(dims) - 1
        rng = np.random.default_rng(9)
        X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
        labels = rng.integers(0, dims[-1], V).astype(np.uint32)
        Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]
        ctx = da.Context(0)
        ctx.configure(da.GCN, dims, V, rank, world)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("halo_exact_rows", exact)
        part.upload(ctx, parts)
        ctx.preallocate()
        ctx.upload(0, "x", X[g["localToGlobal"]])
        if g["srcGhostCnt"]:
            ctx.upload(0, "fg", X[g["srcGhost"]].reshape(g["srcGhostCnt"], dims[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
        ctx.adam_config(0.01)
        seen = []

        def alltoallv(send, sc, so, recv, rc, ro):
            seen.append(tuple([int(x) for x in a] for a in (sc, so, rc, ro)))
            reqs, keep = [], []
            for p in range(world):
                if p == rank:
                    assert sc[p] == 0 and rc[p] == 0
                    continue
                if rc[p]:
                    t = torch.empty(int(rc[p]), dtype=torch.float32)
                    keep.append((t, int(ro[p]), int(rc[p])))
                    reqs.append(dist.irecv(t, p))
                if sc[p]:
                    t = torch.from_numpy(send[int(so[p]):int(so[p] + sc[p])].copy())
                    reqs.append(dist.isend(t, p))
            for r_ in reqs:
                r_.wait()
            for t, o, n in keep:
                recv[o:o + n] = t.numpy()

        def allreduce(buf):
            t = torch.from_numpy(buf.copy())
            dist.all_reduce(t)
            buf[:] = t.numpy()
        ctx.set_host_transport(alltoallv, allreduce)
        eng = da.NativeEngine(ctx)
        eng.run(1)
        ctx.sync()
        res = {"seen": seen, "counters": tuple(int(ctx.get_option(k)) for k in COUNTERS), "tensors": {}, "W": [], "dW": []}
        for l, nm in ((0, "ah"), (1, "ah"), (0, "h"), (0, "aTg"), (1, "grad"), (1, "fg"), (0, "bg")):
            rows = ctx.info(l, nm)[0]
            if rows:
                res["tensors"][(l, nm)] = ctx.download(l, nm)
        for l in range(L):
            res["W"].append(ctx.weight_get(l))
            res["dW"].append(ctx.weight_grad_get(l))
        eng.close()
        ctx.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception:
        q.put((rank, traceback.format_exc()))


def _host_transport_run(exact):
    import torch.multiprocessing as mp
    world = 2
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = _free_port()
    procs = [ctxm.Process(target=_worker, args=(r, world, port, exact, q)) for r in range(world)]
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
    return [r for _, r in res]


def test_host_transport_counts_are_rows_times_cols():
    """two processes on one GPU, the bytes over gloo: the counts and offsets the callback is given are rows x 41 and row offsets
    x 41 floats (rows x 64 with the option 0), and the epoch's tensors, weights and gradients are option 0's bits"""
    exact, padded = _host_transport_run(1), _host_transport_run(0)
    for rank in (0, 1):
        e, p = exact[rank], padded[rank]
        assert len(e["seen"]) == len(p["seen"]) == 2          # one forward, one backward exchange, both of 41-float rows
        for ce, cp in zip(e["seen"], p["seen"]):
            for ae, ap in zip(ce, cp):                        # send counts, send offsets, receive counts, receive offsets
                assert all(x % 64 == 0 for x in ap), (rank, ap)
                assert ae == [x // 64 * 41 for x in ap], (rank, ae, ap)
        assert sum(sum(c[0]) + sum(c[2]) for c in e["seen"]) > 0
        assert e["counters"][0] == p["counters"][0] > 0
        assert e["counters"][1] == e["counters"][0] * 41 and p["counters"][1] == p["counters"][0] * 64
        assert e["counters"][2] == 2 and p["counters"][2] == 0
        assert set(e["tensors"]) == set(p["tensors"])
        for k in e["tensors"]:
            assert np.array_equal(_bits(e["tensors"][k]), _bits(p["tensors"][k])), (rank, k)
        for l in range(2):
            assert np.array_equal(_bits(e["W"][l]), _bits(p["W"][l])) and np.array_equal(_bits(e["dW"][l]), _bits(p["dW"][l])), (rank, l)
    # rank 0's send counts are rank 1's receive counts
    for c0, c1 in zip(exact[0]["seen"], exact[1]["seen"]):
        assert c0[0][1] == c1[2][0] and c1[0][0] == c0[2][1]
