"""dory_gatmh_bwd_merged_exchange (include/dorylus_hip.h): the 8-head GAT's backward sweep ships do and st of a sent vertex as one
merged row [do[v, 0:w) | st[v, 0:4K)] in ONE exchange, and -- with dory_halo_fused_pack on and the sweep forms running -- the
row-wise kernel that produces st writes the send rows itself (csrc/gat_mh_sweep.hip: gatmh_dst_rowwise_send_kernel; the pack and
unpack of merged rows: csrc/elementwise.hip, gather_rows_pair_kernel / scatter_rows_pair_kernel).  Every comparison between the
switch off and on is bit for bit; the reference for the bytes is tests/gatmh_bwd_merged_ref.py.

  1. bytes on the wire: one context, rank 0 of 4, a host transport that records what travels and delivers deterministic rows;
  2. whole epochs over the in-process transport, the switch off against on;
  3. the split entry points (gatmh_bwd_phase = 1 / 2) against the float64 oracle;
  4. not taken (halo_direct_recv plans), and in-process ranks that disagree;
  5. refused arguments, the single partition."""
import ctypes as C
import time

import numpy as np
import pytest

import gatmh_bwd_merged_ref as mr
from test_gpu_gat_mh import RTOL
from test_gpu_halo_fused_pack import _bits, _graph, _send_lists
from test_gpu_halo_fused_pack_rowwise import _same_bits

pytestmark = pytest.mark.gpu
P = 4
RECV = [[], [2], [0], [1]]                      # three ghost rows: peer 1's row lands in slot 2, peer 2's in 0, peer 3's in 1
SLOT_OF_ROW = [2, 0, 1]                         # received row r -> ghost slot
# (hidden layer (K, D), last layer (K, classes)): every shape of the issue once as a hidden layer / as a last layer
MODELS = [((4, 8), (1, 41)), ((4, 16), (2, 8)), ((8, 16), (1, 41)), ((4, 64), (2, 8))]


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _raw(ctx, layer, name):
    """the device tensor as it is stored: [rows, ld], padding included"""
    rows, cols, ld, p = ctx.info(layer, name)
    out = np.zeros((rows, ld), np.float32)
    if rows:
        ctx.sync()
        hip = C.CDLL("libamdhip64.so")
        hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
        assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) == 0
    return out


class Rig:
    """one 8-head GAT context, rank 0 of 4, M local rows and three ghost rows on either side; the host transport records what every
    exchange sends and delivers rows out of fixed tables, whatever the row format of the exchange"""

    def __init__(self, da, M, hidden, last, variant):
        self.da, self.M = da, M
        (K0, D0), (K1, C1) = hidden, last
        self.heads, self.dims = [K0, K1], [12, K0 * D0, C1]
        self.zw = [K0 * D0, K1 * C1]
        ctx = self.ctx = da.Context(0)
        ctx.configure(da.GATMH, self.dims, 4 * M + 8, 0, P)
        ctx.gatmh_heads(self.heads)
        ctx.set_option("spmm_blk_nb", 8)           # the sweep forms on a graph this small
        ctx.graph_upload(_graph(M))
        ctx.preallocate()
        self.lists = _send_lists(M, variant)
        self.total = sum(len(l) for l in self.lists)
        for d in (da.FORWARD, da.BACKWARD):
            ctx.halo_plan(d, self.lists, RECV)
        rng = np.random.default_rng([9, M, K0, D0, K1, C1])
        ctx.upload(0, "h", rng.uniform(-1, 1, (M, self.dims[0])).astype(np.float32))
        ctx.labels_upload(rng.integers(0, C1, M).astype(np.uint32))
        inw = [self.dims[0], self.zw[0]]
        for l in range(2):
            ctx.weight_set(l, "w", (rng.standard_normal((inw[l], self.zw[l])) / np.sqrt(inw[l])).astype(np.float32))
            ctx.weight_set(l, "a_l", (rng.standard_normal(self.zw[l]) * 0.3).astype(np.float32))
            ctx.weight_set(l, "a_r", (rng.standard_normal(self.zw[l]) * 0.3).astype(np.float32))
        # what the peers "send": ghost rows of z, do and st per layer (st: (er, m, 1/den, t) records of moderate size)
        self.gz = [rng.uniform(-1, 1, (3, self.zw[l])).astype(np.float32) for l in range(2)]
        self.gdo = [rng.uniform(-1, 1, (3, self.zw[l])).astype(np.float32) for l in range(2)]
        self.gst = [rng.uniform(0.5, 1.5, (3, 4 * self.heads[l])).astype(np.float32) for l in range(2)]
        self.stage, self.calls, self.n0 = None, [], 0

        def alltoallv(send, sc, so, recv, rc, ro):
            n = int((so + sc).max())
            kind, l = self.stage
            k = len(self.calls) - self.n0                                        # the k-th exchange of this backward pass
            self.calls.append({"stage": self.stage, "send": np.array(send[:n], copy=True), "sc": [int(x) for x in sc], "so": [int(x) for x in so],
                               "rc": [int(x) for x in rc]})
            fl = int(sum(rc)) // 3
            assert fl * 3 == int(sum(rc))
            if kind == "fwd":                                                    # (no library call in here: the exchange holds the context's lock)
                rows = self._wide(self.gz[l], fl)
            elif self.merged:
                R, w, k4 = self.row(l)
                assert fl == R, (fl, R)
                rows = np.concatenate([self._wide(self.gdo[l], w), self.gst[l]], axis=1)
            else:                                                                # the two exchanges: do first, then st
                rows = self._wide(self.gdo[l] if k == 0 else self.gst[l], fl)
            recv[:3 * fl] = rows[SLOT_OF_ROW].reshape(-1)
        ctx.set_host_transport(alltoallv, lambda buf: None)
        self.merged, self.exact = False, 0

    @staticmethod
    def _wide(t, width):
        out = np.zeros((t.shape[0], width), np.float32)
        n = min(width, t.shape[1])
        out[:, :n] = t[:, :n]
        return out

    def row(self, l):
        return mr.wire_row(self.zw[l], self.heads[l], self.exact)

    def forward(self):
        c, da = self.ctx, self.da
        for l in range(2):
            self.stage = ("fwd", l)
            c.apply_vertex(l, da.FORWARD)
            c.halo_exchange(l + 1, da.FORWARD)
            c.apply_edge(l + 1, da.FORWARD)
            c.aggregate(l + 1, da.FORWARD)
        c.predict_gat(2)

    def backward(self, l):
        """the whole backward dory_aggregate of layer l; returns the exchanges it made"""
        from helpers import _poison_padding
        c, da = self.ctx, self.da
        for nm in ("bg_do", "bg_st"):
            _poison_padding(c, l, nm)                                  # the unpack must leave zeros there whatever they held
        self.stage = ("bwd", l)
        n = self.n0 = len(self.calls)
        c.aggregate(l + 1, da.BACKWARD)
        c.sync()
        return self.calls[n:]

    def counters(self):
        c = self.ctx
        return {"merged": np.array(c.gatmh_bwd_merged_exchange_stats(), np.int64), "fused": np.array(c.halo_fused_pack_stats(), np.int64),
                "packed": np.array([int(c.get_option("halo_rows_packed")), int(c.get_option("halo_floats_packed"))], np.int64)}


LOCALS = ("t", "der", "st", "del", "dz", "do")


def _epoch(rig, merged, fused, exact, what):
    """forward, then both backward passes with every check of the wire; returns the bits of what the backward passes leave"""
    ctx, da = rig.ctx, rig.da
    ctx.set_option("halo_exact_rows", exact)
    ctx.halo_fused_pack(fused)
    ctx.gatmh_bwd_merged_exchange(merged)
    rig.merged, rig.exact = bool(merged), exact
    rig.forward()
    out = {}
    for l in (1, 0):
        K, cols = rig.heads[l], rig.zw[l]
        R, w, k4 = rig.row(l)
        assert ctx.gatmh_bwd_wire_row(l) == (R, w, k4), (what, l)
        before = rig.counters()
        calls = rig.backward(l)
        d = {k: (v - before[k]).tolist() for k, v in rig.counters().items()}
        do, st = ctx.download(l, "do"), ctx.download(l, "st")
        T = rig.total
        ld, ld_st = mr.pad_ld(cols), mr.pad_ld(4 * K)
        if merged:
            assert len(calls) == 1, (what, l, "one exchange", len(calls))
            want = mr.pack(do, st, K, w, rig.lists)
            got = calls[0]["send"]
            assert calls[0]["sc"] == [len(x) * R for x in rig.lists], (what, l, calls[0]["sc"])
            assert calls[0]["so"] == [int(x) * R for x in np.cumsum([0] + [len(x) for x in rig.lists[:-1]])], (what, l, calls[0]["so"])
            assert calls[0]["rc"] == [0, R, R, R], (what, l, calls[0]["rc"])
            assert got.size == want.size == T * R, (what, l, got.size, want.size)
            assert np.array_equal(_bits(got), _bits(want)), (what, l, "bytes on the wire", int((_bits(got) != _bits(want)).sum()))
            assert d["merged"] == [1, T, fused, 0], (what, l, d)
            assert d["fused"] == ([1, T, 0] if fused else [0, 0, 0]), (what, l, d)
            assert d["packed"] == ([0, 0] if fused else [T, T * R]), (what, l, d)
        else:
            assert len(calls) == 2, (what, l, "two exchanges", len(calls))
            assert d["merged"] == [0, 0, 0, 0], (what, l, d)
            assert d["fused"] == ([0, 0, 2] if fused else [0, 0, 0]), (what, l, d)
        # the delivered rows, whole ghost rows: the reference's unpack of what the transport handed over
        buf = np.concatenate([Rig._wide(rig.gdo[l], w), rig.gst[l]], axis=1)[SLOT_OF_ROW].reshape(-1)
        want_do, want_st = mr.unpack(buf, K, w, RECV, 3, ld, ld_st)
        assert np.array_equal(_bits(_raw(ctx, l, "bg_do")), _bits(want_do)), (what, l, "bg_do")
        assert np.array_equal(_bits(_raw(ctx, l, "bg_st")), _bits(want_st)), (what, l, "bg_st")
        ctx.apply_vertex(l, da.BACKWARD)
        for nm in LOCALS:
            out[(l, nm)] = _bits(ctx.download(l, nm)).copy()
    return out


@pytest.mark.parametrize("M", [67, 300])
@pytest.mark.parametrize("hidden,last", MODELS, ids=["h%dx%d-l%dx%d" % (h + l) for h, l in MODELS])
def test_one_exchange_of_merged_rows_with_the_references_bytes(da, M, hidden, last):
    """M = 67: a part-filled last workgroup and a wave that ends inside a row group.  Send lists: variant 0 has a row listed for all
    three peers and rows listed for none, variant 1 has a peer with an empty list"""
    for variant in (0, 1):
        rig = Rig(da, M, hidden, last, variant)
        assert rig.ctx.gatmh_bwd_merged_exchange_stats() == (0, 0, 0, 0)
        if variant == 0:
            cnt = np.bincount(np.concatenate([np.unique(l) for l in rig.lists if len(l)]).astype(np.int64), minlength=M)
            assert cnt.max() == 3 and (cnt == 0).any()
        else:
            assert rig.lists[2] == []
        for exact in (0, 1):
            ref = _epoch(rig, 0, 0, exact, (M, variant, exact, "off"))
            for fused in (0, 1):
                got = _epoch(rig, 1, fused, exact, (M, variant, exact, "on", fused))
                for k in ref:
                    assert np.array_equal(ref[k], got[k]), (M, variant, exact, fused, k, "the switch off against on")
        _epoch(rig, 0, 1, 0, (M, variant, "off, dory_halo_fused_pack on: two counted fallbacks"))
        rig.ctx.close()


# ---- 2. whole epochs over the in-process transport ----------------------------------------------------------------------------------
def _parts(da, Pn, V=240, E=2600):
    """the graph of test_local_transport_gat_mh_epoch_vs_oracle: a hub destination and a hub source, scattered ownership"""
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % Pn).astype(np.int32)
    return s, d, parts, rng


def _epochs(da, Pn, dims, heads, epochs, merged, fused, opts=None, only_rank=None):
    """run_local of the multi-head GAT with the switch as asked (only_rank: on that rank alone); (result, {rank: counters})"""
    from local_ranks import run_local
    s, d, parts, rng = _parts(da, Pn)
    V, L = len(parts), len(dims) - 1
    pobjs = [da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, Pn) for r in range(Pn)]
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    zw = [dims[l + 1] * (heads[l] if l == L - 1 else 1) for l in range(L)]
    inw = [dims[0]] + zw[:-1]
    Ws = [(rng.standard_normal((inw[l], zw[l])) / np.sqrt(inw[l])).astype(np.float32) for l in range(L)]
    Al = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
    Ar = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l in range(L):
            ctx.weight_set(l, "w", Ws[l])
            ctx.weight_set(l, "a_l", Al[l])
            ctx.weight_set(l, "a_r", Ar[l])
        ctx.halo_fused_pack(fused)
        ctx.gatmh_bwd_merged_exchange(merged if only_rank is None or r == only_rank else 0)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"merged": ctx.gatmh_bwd_merged_exchange_stats(), "fused": ctx.halo_fused_pack_stats(),
                           "made": int(ctx.get_option("halo_direct_recvs")) + int(ctx.get_option("halo_staged_recvs"))}
            close()
        ctx.close = closing
    dl = [(l, nm) for l in range(L) for nm in ("z", "o", "t", "del", "der", "dz", "fg_z", "bg_do", "bg_st")] + [(L - 1, "logits")]
    out = run_local(da, pobjs, parts, dims, da.GATMH, epochs, setup, dict({"spmm_blk_nb": 8}, **(opts or {})), downloads=dl,
                    pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r"))
    return out, kept


@pytest.mark.parametrize("Pn", [2, 4])
@pytest.mark.parametrize("dims,heads,packed_layers", [([40, 128, 41], [8, 1], 2), ([24, 64, 6], [4, 1], 1)], ids=["40-128-41", "24-64-6"])
def test_epochs_switch_off_against_on(da, Pn, dims, heads, packed_layers):
    """two epochs; 24-64-6: the last layer's backward (one head of 6 features) takes the blocked kernels -- the pair kernel packs
    there, the producer packs on the hidden layer"""
    epochs, L = 2, 2
    off, koff = _epochs(da, Pn, dims, heads, epochs, 0, 0)
    for fused in (0, 1):
        on, kon = _epochs(da, Pn, dims, heads, epochs, 1, fused)
        what = (Pn, dims, "fused", fused)
        _same_bits(off, on, what)
        assert set(koff) == set(kon) == set(range(Pn))
        for r in range(Pn):
            assert koff[r]["merged"] == (0, 0, 0, 0), (what, r, koff[r])
            assert koff[r]["made"] - kon[r]["made"] == L * epochs, (what, r, koff[r], kon[r])
            m = kon[r]["merged"]
            assert m[0] == L * epochs and m[3] == 0, (what, r, m)
            assert m[2] == (packed_layers * epochs if fused else 0), (what, r, m)
            f = kon[r]["fused"]
            assert (f[0] + f[2] == kon[r]["made"]) if fused else (f == (0, 0, 0)), (what, r, kon[r])


# ---- 3. the split entry points against the float64 oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("dims,heads", [([24, 64, 6], [4, 1]), ([24, 128, 6], [8, 1])])
@pytest.mark.parametrize("Pn,exact", [(2, 0), (4, 1)])
def test_split_entry_points_vs_oracle(da, Pn, dims, heads, exact):
    """the arrangement of test_gat_mh_partitioned_epoch_vs_oracle (one context per partition, gatmh_bwd_phase 1 / 2, device copies
    between the contexts) with ONE gatmh_bwd_pack / gatmh_bwd_unpack round in place of the two halo_pack_tensor rounds; that test's
    tolerances"""
    import torch
    import gat_mh_oracle as go
    import partition_oracle as po
    from halo_plan_ref import halo_plan
    from helpers import rel_err
    V, E = 240, 2600
    s, d, parts, rng = _parts(da, Pn, V, E)
    parts = parts.astype(np.int64)
    g_all = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
    gs = [po.preprocess(s, d, parts, r, Pn) for r in range(Pn)]
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = []
    for l in range(2):
        zw = dims[l + 1] * (heads[l] if l == 1 else 1)
        params.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                       (rng.standard_normal(zw) * 0.3).astype(np.float32), (rng.standard_normal(zw) * 0.3).astype(np.float32)])
    ctxs, plans = [], []
    for r, g in enumerate(gs):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V, r, Pn)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("halo_exact_rows", exact)
        ctx.graph_upload(g)
        with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_pack"):
            ctx.gatmh_bwd_pack(0, 0)                                    # before dory_preallocate
        ctx.preallocate()
        with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_wire_row"):
            ctx.gatmh_bwd_wire_row(0)                                   # no backward plan yet
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        pl = halo_plan(g, parts, r, Pn)
        for dd in (0, 1):
            ctx.halo_plan(dd, pl[dd][0], pl[dd][1])
        ctxs.append(ctx)
        plans.append(pl)

    def route(send, recv, dd, fl):
        for r in range(Pn):
            soff = np.concatenate([[0], np.cumsum([len(x) for x in plans[r][dd][0]])])
            for p in range(Pn):
                roff = np.concatenate([[0], np.cumsum([len(x) for x in plans[p][dd][1]])])
                n = len(plans[r][dd][0][p])
                recv[p][roff[r] * fl:(roff[r] + n) * fl] = send[r][soff[p] * fl:(soff[p] + n) * fl]
        torch.cuda.synchronize()

    def bufs(dd, fl):
        send = [torch.zeros(max(1, sum(len(x) for x in plans[r][dd][0])) * fl, device="cuda") for r in range(Pn)]
        recv = [torch.zeros(max(1, sum(len(x) for x in plans[r][dd][1])) * fl, device="cuda") for r in range(Pn)]
        torch.cuda.synchronize()
        return send, recv

    def exchange_z(layer):
        fl = ctxs[0].info(layer, "z", ptr=False)[1 if exact else 2]      # (exact rows: cols floats)
        send, recv = bufs(0, fl)
        for r in range(Pn):
            ctxs[r].halo_pack_tensor(layer, "z", 0, send[r].data_ptr())
            ctxs[r].sync()
        route(send, recv, 0, fl)
        for r in range(Pn):
            ctxs[r].halo_unpack_tensor(layer, "fg_z", 0, recv[r].data_ptr())
            ctxs[r].sync()

    def exchange_do_st(layer):
        K = heads[layer]
        zw = dims[layer + 1] * (K if layer == 1 else 1)
        rows = {c.gatmh_bwd_wire_row(layer) for c in ctxs}
        assert rows == {mr.wire_row(zw, K, exact)}, rows
        R = rows.pop()[0]
        send, recv = bufs(1, R)
        for r in range(Pn):
            ctxs[r].gatmh_bwd_pack(layer, send[r].data_ptr())
            ctxs[r].sync()
        route(send, recv, 1, R)
        for r in range(Pn):
            ctxs[r].gatmh_bwd_unpack(layer, recv[r].data_ptr())
            ctxs[r].sync()

    L = 2
    for l in range(L):
        for c in ctxs:
            c.apply_vertex(l, da.FORWARD)
        exchange_z(l)
        for c in ctxs:
            c.apply_edge(l + 1, da.FORWARD)
            c.aggregate(l + 1, da.FORWARD)
    for c in ctxs:
        c.predict_gat(L)
    for l in range(L - 1, -1, -1):
        for c in ctxs:
            c.set_option("gatmh_bwd_phase", 1)
            c.aggregate(l + 1, da.BACKWARD)
        exchange_do_st(l)
        for c in ctxs:
            c.set_option("gatmh_bwd_phase", 2)
            c.aggregate(l + 1, da.BACKWARD)
            c.apply_vertex(l, da.BACKWARD)
    fws, Hs, loss, dlogits, grads = go.epoch(g_all, X, labels, [[p.astype(np.float64) for p in ps] for ps in params], heads)

    def gathered(layer, name):
        out = None
        for r, g in enumerate(gs):
            t = ctxs[r].download(layer, name)
            if out is None:
                out = np.zeros((V, t.shape[1]), np.float32)
            out[g["localToGlobal"]] = t
        return out
    for l in range(L):
        assert rel_err(gathered(l, "z"), fws[l]["Z"]) < RTOL, (l, "z")
        assert rel_err(gathered(l, "o"), fws[l]["O"]) < RTOL, (l, "o")
        assert rel_err(gathered(l, "t"), grads[l]["t"]) < 5e-4, (l, "t")
        assert rel_err(gathered(l, "del"), grads[l]["d_el"]) < 5e-4, (l, "del")
        assert rel_err(gathered(l, "der"), grads[l]["d_er"]) < 5e-4, (l, "der")
        assert rel_err(gathered(l, "dz"), grads[l]["dZ"]) < 5e-4, (l, "dz")
        assert rel_err(sum(c.weight_grad_get(l, "w") for c in ctxs), grads[l]["dW"]) < 5e-4, (l, "dW")
        assert rel_err(sum(c.weight_grad_get(l, "a_l") for c in ctxs).ravel(), grads[l]["da_l"]) < 5e-4, (l, "da_l")
        assert rel_err(sum(c.weight_grad_get(l, "a_r") for c in ctxs).ravel(), grads[l]["da_r"]) < 5e-4, (l, "da_r")
    assert rel_err(gathered(1, "logits"), Hs[2]) < RTOL
    for c in ctxs:
        assert c.gatmh_bwd_merged_exchange_stats() == (0, 0, 0, 0)          # (the library exchanged nothing)
        c.close()


# ---- 4. not taken; ranks that disagree -------------------------------------------------------------------------------------------------
def test_direct_recv_plans_keep_the_two_exchanges(da):
    dims, heads, epochs, L = [40, 128, 41], [8, 1], 2, 2
    off, koff = _epochs(da, 2, dims, heads, epochs, 0, 1, {"halo_direct_recv": 1})
    on, kon = _epochs(da, 2, dims, heads, epochs, 1, 1, {"halo_direct_recv": 1})
    _same_bits(off, on, "halo_direct_recv = 1")
    for r in range(2):
        assert koff[r]["merged"] == (0, 0, 0, 0), (r, koff[r])
        assert kon[r]["merged"] == (0, 0, 0, L * epochs), (r, kon[r])
        assert kon[r]["made"] == koff[r]["made"] and kon[r]["fused"] == koff[r]["fused"], (r, kon[r], koff[r])


def test_local_ranks_that_disagree_fail_at_once(da):
    """rank 0 with the switch on, rank 1 off: the backward pass that checks first fails with DORY_ERR_COMM naming both ranks before
    anything of its exchange is enqueued; nothing hangs (local_timeout_ms = 300 as the transport's own timeout test sets it)"""
    dims, heads = [24, 64, 6], [4, 1]
    s, d, parts, rng = _parts(da, 2)
    V = len(parts)
    ctxs = []
    for r in range(2):
        part = da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, 2)
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V, r, 2)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("local_timeout_ms", 300)
        part.upload(ctx, parts)
        ctx.preallocate()
        g = part.view()
        ctx.upload(0, "h", rng.uniform(-1, 1, (int(g["localVtxCnt"]), dims[0])).astype(np.float32))
        ctx.labels_upload(rng.integers(0, dims[-1], int(g["localVtxCnt"])).astype(np.uint32))
        ctx.weights_init_xavier()
        ctx.gatmh_bwd_merged_exchange(1 - r)
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    for l in range(2):                                                   # stage by stage: every rank's exchange before any rank's consumer
        for c in ctxs:
            c.apply_vertex(l, da.FORWARD)
            c.halo_exchange(l + 1, da.FORWARD)
        for c in ctxs:
            c.apply_edge(l + 1, da.FORWARD)
            c.aggregate(l + 1, da.FORWARD)
    for c in ctxs:
        c.predict_gat(2)
    for r in (0, 1):
        t0 = time.perf_counter()
        with pytest.raises(da.DoryError, match=r"error -4.*gatmh_bwd_merged_exchange differs.*rank %d has %d.*rank %d has %d" % (r, 1 - r, 1 - r, r)):
            ctxs[r].aggregate(2, da.BACKWARD)
        assert time.perf_counter() - t0 < 1.0
        assert ctxs[r].gatmh_bwd_merged_exchange_stats() == (0, 0, 0, 0)
    for c in ctxs:
        c.close()


# ---- 5. refused arguments, the single partition -------------------------------------------------------------------------------------------
def test_refused_arguments_and_single_partition(da):
    import aggregate_ref as ar
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_merged_exchange"):
        c.gatmh_bwd_merged_exchange(1)                                 # before dory_configure
    c.configure(da.GCN, [4, 41, 2], 100, 0, 2)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_merged_exchange.*DORY_GATMH"):
        c.gatmh_bwd_merged_exchange(1)                                 # a GCN context
    for fn in (lambda: c.gatmh_bwd_wire_row(0), lambda: c.gatmh_bwd_pack(0, 0), lambda: c.gatmh_bwd_unpack(0, 0)):
        with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_"):
            fn()
    c.close()
    c = da.Context(0)
    c.configure(da.GATMH, [16, 32, 4], 100, 0, 2)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_merged_exchange"):
            c.gatmh_bwd_merged_exchange(bad)
    for fn in (lambda: c.gatmh_bwd_wire_row(0), lambda: c.gatmh_bwd_pack(0, 0), lambda: c.gatmh_bwd_unpack(0, 0)):
        with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_.*dory_preallocate"):
            fn()                                                       # the split entry points before dory_preallocate
    c.gatmh_bwd_merged_exchange(1)                                     # any time after dory_configure
    c.gatmh_bwd_merged_exchange(0)
    assert c.gatmh_bwd_merged_exchange_stats() == (0, 0, 0, 0)
    c.close()
    # a single partition: accepted and inert -- an epoch matches the switch-off run bit for bit, the counters stay 0; refused while
    # an epoch graph is being recorded
    g = ar.graph("uniform:200:1500")
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (200, 16)).astype(np.float32)
    labels = rng.integers(0, 4, 200).astype(np.uint32)
    runs = []
    for on in (0, 1):
        one = da.Context(0)
        one.configure(da.GATMH, [16, 32, 4], 200)
        one.gatmh_heads([4, 1])
        one.set_option("spmm_blk_nb", 8)
        one.graph_upload(g)
        one.preallocate()
        one.upload(0, "h", X)
        one.labels_upload(labels)
        wr = np.random.default_rng(8)
        for l, (fi, fo) in enumerate(((16, 32), (32, 4))):
            one.weight_set(l, "w", (wr.standard_normal((fi, fo)) / np.sqrt(fi)).astype(np.float32))
            one.weight_set(l, "a_l", (wr.standard_normal(fo) * 0.3).astype(np.float32))
            one.weight_set(l, "a_r", (wr.standard_normal(fo) * 0.3).astype(np.float32))
        one.halo_fused_pack(1)
        one.gatmh_bwd_merged_exchange(on)
        one.adam_config(0.01)
        eng = da.NativeEngine(one)
        eng.run(1)
        one.sync()
        assert one.gatmh_bwd_merged_exchange_stats() == (0, 0, 0, 0) and one.halo_fused_pack_stats() == (0, 0, 0)
        runs.append({"t": {(l, nm): _bits(one.download(l, nm)) for l in range(2) for nm in ("z", "o", "t", "der", "del", "dz")},
                     "W": [_bits(one.weight_get(l, nm)) for l in range(2) for nm in ("w", "a_l", "a_r")]})
        eng.close()
        if on:
            one.epoch_graph_begin()
            with pytest.raises(da.DoryError, match="error -1.*epoch graph is being recorded"):
                one.gatmh_bwd_merged_exchange(0)
            one.epoch_graph_drop()
            one.gatmh_bwd_merged_exchange(0)
        one.close()
    for k in runs[0]["t"]:
        assert np.array_equal(runs[0]["t"][k], runs[1]["t"][k]), k
    for a, b in zip(runs[0]["W"], runs[1]["W"]):
        assert np.array_equal(a, b)
