"""dory_gatmh_halo_bf16 (include/dorylus_hip.h): on top of dory_halo_bf16_rows the 8-head GAT ships z -> fg_z as bf16 rows while
gatmh_bf16_gather >= 1 and the backward sweep's do while it is 2 -- alone through the bf16 pack / unpack, or inside the merged row
[do as bf16 | st as fp32] of dory_gatmh_bwd_merged_exchange (csrc/elementwise.hip: gather_rows_pair_bf16_kernel /
scatter_rows_pair_bf16_kernel; csrc/gat_mh_sweep.hip: gatmh_dst_rowwise_send_bf16_kernel); st always travels fp32.  The reference for
the bytes is tests/gatmh_halo_bf16_ref.py (merged rows) and tests/halo_bf16_ref.py (bf16 rows); every comparison of results is bit for
bit against a run with the switch off that is DELIVERED the rounded ghost rows as fp32.

  1. bytes and bits: one context, rank 0 of 4, a host transport that records what travels and delivers deterministic rows;
  2. the split entry points (gatmh_bwd_phase = 1 / 2, dory_halo_pack) against the reference bytes;
  3. whole epochs over the in-process transport;
  4. not taken (halo_direct_recv plans, the scatter transport, dory_halo_pack_tensor), ranks that disagree, refusals, inert cases;
  5. a replayed epoch graph."""
import threading

import numpy as np
import pytest

import gatmh_bwd_merged_ref as mr
import gatmh_halo_bf16_ref as gr
import halo_bf16_ref as hb
from test_gpu_gatmh_bf16_gather import EL_TABLE_LAYERS, backward_takes_the_sweep_forms
from test_gpu_gatmh_bwd_merged import LOCALS, MODELS, RECV, SLOT_OF_ROW, Rig, _raw
from test_gpu_halo_bf16_rows import _check_ghosts, _own_views
from test_gpu_halo_fused_pack import _bits, _golden

pytestmark = pytest.mark.gpu
FWD, BWD = 0, 1


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _f32(u16_rows):
    """rows of uint16 as the float32 words that hold them"""
    return np.ascontiguousarray(u16_rows, np.uint16).view(np.float32)


def _u16(f32):
    return np.ascontiguousarray(f32, np.float32).view(np.uint16)


# ---- 1. bytes and bits, one context ---------------------------------------------------------------------------------------------------
class Rig16(Rig):
    """the rig of tests/test_gpu_gatmh_bwd_merged.py with a host transport that also delivers bf16 rows: fwd16 / do16 say what the
    exchange of the moment ships (the peers pack by the same rule), round_fwd / round_do make it deliver the ROUNDED rows as fp32 --
    what the comparison run gets"""

    def __init__(self, da, M, hidden, last, variant):
        super().__init__(da, M, hidden, last, variant)
        self.fwd16 = self.do16 = self.round_fwd = self.round_do = False
        three = [[0, 1, 2]]

        def alltoallv(send, sc, so, recv, rc, ro):
            n = int((so + sc).max())
            kind, l = self.stage
            k = len(self.calls) - self.n0
            self.calls.append({"stage": self.stage, "send": np.array(send[:n], copy=True), "sc": [int(x) for x in sc], "so": [int(x) for x in so],
                               "rc": [int(x) for x in rc]})
            fl = int(sum(rc)) // 3
            assert fl * 3 == int(sum(rc))
            K, cols = self.heads[l], self.zw[l]
            gz = hb.rounded(self.gz[l]) if self.round_fwd else self.gz[l]
            gdo = hb.rounded(self.gdo[l]) if self.round_do else self.gdo[l]
            if kind == "fwd":
                rows = _f32(hb.pack(self.gz[l], three[0], cols, self.exact).reshape(3, -1)) if self.fwd16 else Rig._wide(gz, fl)
            elif self.merged and self.do16:
                R, dof, k4, w = gr.wire_row(cols, K, self.exact)
                rows = gr.pack(self.gdo[l], self.gst[l], K, w, three).reshape(3, R)
            elif self.merged:
                R, w, k4 = mr.wire_row(cols, K, self.exact)
                rows = np.concatenate([Rig._wide(gdo, w), self.gst[l]], axis=1)
            elif k == 0:                                                         # the two exchanges: do first, then st
                rows = _f32(hb.pack(self.gdo[l], three[0], cols, self.exact).reshape(3, -1)) if self.do16 else Rig._wide(gdo, fl)
            else:
                rows = Rig._wide(self.gst[l], fl)
            assert rows.shape == (3, fl), (self.stage, k, rows.shape, fl)
            recv[:3 * fl] = rows[SLOT_OF_ROW].reshape(-1)
        self.ctx.set_host_transport(alltoallv, lambda buf: None)

    def ids(self):
        return np.concatenate([np.asarray(x, np.int64) for x in self.lists if len(x)])

    def counters16(self):
        c = self.ctx
        d = self.counters()
        d["gat16"] = np.array(c.gatmh_halo_bf16_stats(), np.int64)
        d["bf16"] = np.array(c.halo_bf16_rows_stats(), np.int64)
        return d


def _set(rig, switch, mode, merged, fused, exact, rows=1):
    ctx = rig.ctx
    ctx.set_option("gatmh_bf16_gather", mode)
    ctx.set_option("halo_exact_rows", exact)
    ctx.halo_fused_pack(fused)
    ctx.halo_fused_pack_bf16(fused)
    ctx.gatmh_bwd_merged_exchange(merged)
    ctx.halo_bf16_rows(rows)
    ctx.gatmh_halo_bf16(switch)
    rig.merged, rig.exact = bool(merged), exact
    rig.fwd16, rig.do16 = bool(switch and rows and mode >= 1), bool(switch and rows and mode == 2)
    rig.round_fwd, rig.round_do = mode >= 1 and not rig.fwd16, mode == 2 and not rig.do16


def _run(rig, switch, mode, merged, fused, exact, what, rows=1):
    """one forward and both backward passes with every check of the wire and the counters; the bits of what they leave"""
    ctx, da = rig.ctx, rig.da
    _set(rig, switch, mode, merged, fused, exact, rows)
    T, ids, out = rig.total, rig.ids(), {}
    lens = [len(x) for x in rig.lists]
    offs = [int(x) for x in np.cumsum([0] + lens[:-1])]
    for l in range(2):
        cols = rig.zw[l]
        rig.stage = ("fwd", l)
        before = rig.counters16()
        ctx.apply_vertex(l, da.FORWARD)
        n = len(rig.calls)
        ctx.halo_exchange(l + 1, da.FORWARD)
        calls = rig.calls[n:]
        d = {k: (v - before[k]).tolist() for k, v in rig.counters16().items()}
        z = ctx.download(l, "z")
        assert len(calls) == 1, (what, l)
        if rig.fwd16:
            re = hb.row_elems(cols, exact)
            assert ctx.halo_wire_row(l + 1, da.FORWARD) == (2, re), (what, l)
            want = hb.pack(z, ids, cols, exact)
            got = _u16(calls[0]["send"])
            assert calls[0]["sc"] == [x * re // 2 for x in lens] and calls[0]["so"] == [x * re // 2 for x in offs], (what, l, calls[0]["sc"])
            assert got.size == want.size == T * re and np.array_equal(got, want), (what, l, "forward bytes", int((got != want).sum()))
            assert d["gat16"] == [1, 0, 0, 0] and d["bf16"] == [1, T * re * 2, 0], (what, l, d)
            assert d["fused"] == ([1, T, 0] if fused else [0, 0, 0]) and d["packed"] == ([0, 0] if fused else [T, T * re // 2]), (what, l, d)
        else:
            w = cols if exact else mr.pad_ld(cols)
            assert ctx.halo_wire_row(l + 1, da.FORWARD) == (4, w), (what, l)
            want = Rig._wide(z, w)[ids] if w % 4 == 0 or not exact else z[ids, :cols]
            assert np.array_equal(_bits(calls[0]["send"]), _bits(want.reshape(-1))), (what, l, "forward fp32 bytes")
            assert d["gat16"] == [0, 0, 0, 0] and d["bf16"] == [0, 0, 1 if rows else 0], (what, l, d)
        ctx.apply_edge(l + 1, da.FORWARD)
        ctx.aggregate(l + 1, da.FORWARD)
    ctx.predict_gat(2)
    for l in range(2):
        for nm in ("fg_z", "fg_el", "o", "op"):
            out[(l, nm)] = _bits(ctx.download(l, nm)).copy()
    out[(1, "logits")] = _bits(ctx.download(1, "logits")).copy()
    for l in (1, 0):
        K, cols = rig.heads[l], rig.zw[l]
        ld_st = mr.pad_ld(4 * K)
        before = rig.counters16()
        calls = rig.backward(l)
        d = {k: (v - before[k]).tolist() for k, v in rig.counters16().items()}
        do, st = ctx.download(l, "do"), ctx.download(l, "st")
        wst = 4 * K if exact else ld_st
        if rig.do16:
            R, dof, k4, w = gr.wire_row(cols, K, exact)
            re = hb.row_elems(cols, exact)
            assert ctx.gatmh_bwd_wire_row(l) == (R, dof, k4) and ctx.gatmh_bwd_wire_do(l) == (2, w), (what, l)
            assert d["gat16"] == [0, 1, T, 1 if merged and fused else 0], (what, l, d)
            if merged:
                assert len(calls) == 1, (what, l, len(calls))
                want, got = gr.pack(do, st, K, w, rig.lists), calls[0]["send"]
                assert calls[0]["sc"] == [x * R for x in lens] and calls[0]["so"] == [x * R for x in offs] and calls[0]["rc"] == [0, R, R, R], (what, l)
                assert got.size == want.size == T * R and np.array_equal(_bits(got), _bits(want)), (what, l, "merged bytes", int((_bits(got) != _bits(want)).sum()))
                assert d["merged"] == [1, T, fused, 0] and d["fused"] == ([1, T, 0] if fused else [0, 0, 0]), (what, l, d)
                assert d["packed"] == ([0, 0] if fused else [T, T * R]) and d["bf16"] == [1, T * R * 4, 0], (what, l, d)
            else:
                assert len(calls) == 2, (what, l, len(calls))
                want = hb.pack(do, ids, cols, exact)
                assert np.array_equal(_u16(calls[0]["send"]), want), (what, l, "do bytes")
                assert calls[0]["sc"] == [x * re // 2 for x in lens] and calls[1]["sc"] == [x * wst for x in lens], (what, l)
                assert np.array_equal(_bits(calls[1]["send"]), _bits(Rig._wide(st, wst)[ids].reshape(-1))), (what, l, "st bytes")
                assert d["merged"] == [0, 0, 0, 0] and d["fused"] == ([0, 0, 2] if fused else [0, 0, 0]), (what, l, d)
                assert d["packed"] == [2 * T, T * re // 2 + T * wst] and d["bf16"] == [1, T * re * 2, 1], (what, l, d)
        else:
            R, w, k4 = mr.wire_row(cols, K, exact)
            assert ctx.gatmh_bwd_wire_row(l) == (R, w, k4) and ctx.gatmh_bwd_wire_do(l) == (4, w), (what, l)
            assert d["gat16"] == [0, 0, 0, 0], (what, l, d)
            assert len(calls) == (1 if merged else 2), (what, l, len(calls))
            if merged:
                assert np.array_equal(_bits(calls[0]["send"]), _bits(mr.pack(do, st, K, w, rig.lists))), (what, l, "fp32 merged bytes")
                assert d["merged"] == [1, T, fused, 0] and d["packed"] == ([0, 0] if fused else [T, T * R]), (what, l, d)
            assert d["bf16"] == [0, 0, (1 if merged else 2) if rows else 0], (what, l, d)
        out[(l, "bg_do")], out[(l, "bg_st")] = _bits(_raw(ctx, l, "bg_do")).copy(), _bits(_raw(ctx, l, "bg_st")).copy()
        ctx.apply_vertex(l, da.BACKWARD)
        for nm in LOCALS:
            out[(l, nm)] = _bits(ctx.download(l, nm)).copy()
        for nm in ("w", "a_l", "a_r"):
            out[(l, "d" + nm)] = _bits(ctx.weight_grad_get(l, nm)).copy()
    return out


def _same(ref, got, what):
    assert set(ref) == set(got), what
    for k in ref:
        assert ref[k].shape == got[k].shape and np.array_equal(ref[k], got[k]), (what, k, int((ref[k] != got[k]).sum()))


ONE = [(67, 0, m) for m in MODELS] + [(300, 1, MODELS[2])]


@pytest.mark.parametrize("M,variant,model", ONE, ids=["M%d-v%d-h%dx%d-l%dx%d" % ((M, v) + m[0] + m[1]) for M, v, m in ONE])
def test_bytes_on_the_wire_and_bits_against_rounded_fp32_delivery(da, M, variant, model):
    """M = 67: a part-filled last workgroup; send lists: a row for all three peers, rows for none, a row twice in one list; variant 1:
    a peer with an empty list.  Every layer of these models takes the sweep forms in its backward, so value 2 is accepted."""
    hidden, last = model
    assert backward_takes_the_sweep_forms(*hidden) and backward_takes_the_sweep_forms(*last)
    rig = Rig16(da, M, hidden, last, variant)
    assert rig.ctx.gatmh_halo_bf16_stats() == (0, 0, 0, 0)
    for exact in (0, 1):
        ref = _run(rig, 0, 2, 0, 0, exact, (M, exact, "off, rounded rows delivered as fp32"))
        for l in range(2):
            assert not (ref[(l, "bg_do")] & 0xFFFF).any() and not (ref[(l, "fg_z")] & 0xFFFF).any()
        for merged, fused, form in ((1, 1, "merged, producer-packed"), (1, 0, "merged, pair kernel"), (0, 0, "two exchanges")):
            _same(ref, _run(rig, 1, 2, merged, fused, exact, (M, exact, "on", form)), (M, exact, form))
        # value 1: forward bf16, the backward's do fp32 -- bg_do unrounded
        ref1 = _run(rig, 0, 1, 0, 0, exact, (M, exact, "value 1, off"))
        got1 = _run(rig, 1, 1, 1, 1, exact, (M, exact, "value 1, on"))
        _same(ref1, got1, (M, exact, "value 1"))
        for l in range(2):
            assert (got1[(l, "bg_do")] & 0xFFFF).any() and not (got1[(l, "fg_z")] & 0xFFFF).any(), (l, "value 1: do travels fp32")
    # dory_halo_bf16_rows off: the switch is inert -- fp32 bytes, and no counter of either feature moves (checked inside _run)
    _same(_run(rig, 0, 2, 1, 1, 0, "rows off, switch off", rows=0), _run(rig, 1, 2, 1, 1, 0, "rows off, switch on", rows=0), "rows off")
    assert rig.ctx.halo_bf16_rows_stats()[0] > 0
    rig.ctx.close()


# ---- 2. the split entry points ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hidden,last", MODELS, ids=["h%dx%d-l%dx%d" % (h + l) for h, l in MODELS])
def test_split_entry_points_give_the_reference_bytes(da, hidden, last):
    """gatmh_bwd_phase 1 / 2 with dory_gatmh_bwd_wire_row / _wire_do / _pack / _unpack in between, and dory_halo_wire_row / _pack for
    the forward: a caller's own transport gets the rows the library's exchange ships"""
    import torch
    from helpers import _poison_padding
    rig = Rig16(da, 67, hidden, last, 0)
    ctx, T, ids = rig.ctx, rig.total, rig.ids()
    for exact in (0, 1):
        _set(rig, 1, 2, 1, 0, exact)
        for l in range(2):
            rig.stage = ("fwd", l)
            ctx.apply_vertex(l, da.FORWARD)
            cols = rig.zw[l]
            re = hb.row_elems(cols, exact)
            assert ctx.halo_wire_row(l + 1, da.FORWARD) == (2, re)
            buf = torch.zeros(T * re // 2, device="cuda")
            torch.cuda.synchronize()
            ctx.halo_pack(l + 1, da.FORWARD, buf.data_ptr())
            ctx.sync()
            assert np.array_equal(_u16(buf.cpu().numpy()), hb.pack(ctx.download(l, "z"), ids, cols, exact)), (exact, l, "halo_pack")
            ctx.halo_exchange(l + 1, da.FORWARD)
            ctx.apply_edge(l + 1, da.FORWARD)
            ctx.aggregate(l + 1, da.FORWARD)
        ctx.predict_gat(2)
        for l in (1, 0):
            K, cols = rig.heads[l], rig.zw[l]
            ld, ld_st = mr.pad_ld(cols), mr.pad_ld(4 * K)
            ctx.set_option("gatmh_bwd_phase", 1)
            ctx.aggregate(l + 1, da.BACKWARD)
            R, dof, k4, w = gr.wire_row(cols, K, exact)
            assert ctx.gatmh_bwd_wire_row(l) == (R, dof, k4) and ctx.gatmh_bwd_wire_do(l) == (2, w), (exact, l)
            before = np.array(ctx.halo_bf16_rows_stats(), np.int64)
            send = torch.zeros(T * R, device="cuda")
            torch.cuda.synchronize()
            ctx.gatmh_bwd_pack(l, send.data_ptr())
            ctx.sync()
            want = gr.pack(ctx.download(l, "do"), ctx.download(l, "st"), K, w, rig.lists)
            assert np.array_equal(_bits(send.cpu().numpy()), _bits(want)), (exact, l, "gatmh_bwd_pack")
            assert (np.array(ctx.halo_bf16_rows_stats(), np.int64) - before).tolist() == [1, T * R * 4, 0], (exact, l)
            rows = gr.pack(rig.gdo[l], rig.gst[l], K, w, [[0, 1, 2]]).reshape(3, R)[SLOT_OF_ROW].reshape(-1)
            recv = torch.from_numpy(rows.copy()).cuda()
            torch.cuda.synchronize()
            for nm in ("bg_do", "bg_st"):
                _poison_padding(ctx, l, nm)
            ctx.gatmh_bwd_unpack(l, recv.data_ptr())
            ctx.sync()
            want_do, want_st = gr.unpack(rows, K, w, RECV, 3, ld, ld_st)
            assert np.array_equal(_bits(_raw(ctx, l, "bg_do")), _bits(want_do)), (exact, l, "bg_do")
            assert np.array_equal(_bits(_raw(ctx, l, "bg_st")), _bits(want_st)), (exact, l, "bg_st")
            ctx.set_option("gatmh_bwd_phase", 2)
            ctx.aggregate(l + 1, da.BACKWARD)
            ctx.apply_vertex(l, da.BACKWARD)
            # with the gather value at 1 the same entry points answer fp32 rows
            ctx.set_option("gatmh_bf16_gather", 1)
            assert ctx.gatmh_bwd_wire_row(l) == mr.wire_row(cols, K, exact) and ctx.gatmh_bwd_wire_do(l) == (4, mr.wire_w(cols, exact)), (exact, l)
            ctx.set_option("gatmh_bf16_gather", 2)
        ctx.set_option("gatmh_bwd_phase", 0)
    # dory_halo_pack_tensor: the consumer is unknown -- fp32 rows, counted while the switch is on
    before = np.array(ctx.halo_bf16_rows_stats(), np.int64)
    ctx.set_option("halo_exact_rows", 0)
    ld = mr.pad_ld(rig.zw[0])
    buf = torch.zeros(T * ld, device="cuda")
    torch.cuda.synchronize()
    ctx.halo_pack_tensor(0, "z", da.FORWARD, buf.data_ptr())
    ctx.sync()
    assert np.array_equal(_bits(buf.cpu().numpy()), _bits(Rig._wide(ctx.download(0, "z"), ld)[ids].reshape(-1)))
    assert (np.array(ctx.halo_bf16_rows_stats(), np.int64) - before).tolist() == [0, 0, 1]
    ctx.close()


# ---- 3. epochs over the in-process transport (and 4: the transports that keep fp32) ------------------------------------------------------
DIMS, HEADS, MODE = [20, 128, 6], [8, 1], 2
ZW = [128, 6]
# the last layer (one head of 6 features) leaves the sweep forms in its backward (backward_takes_the_sweep_forms), where value 2 is
# refused: its backward runs with value 1 -- the option is read per call -- and ships its do in fp32
BWD_VALUE = [2 if backward_takes_the_sweep_forms(HEADS[l], ZW[l] // HEADS[l]) else 1 for l in range(2)]
DL = [(l, nm) for l in range(2) for nm in ("z", "o", "op", "t", "del", "der", "dz", "do", "st", "fg_z", "fg_el", "bg_do", "bg_st")] + [(1, "logits")]


def _drive(da, case, switch, fused=0, merged=0, epochs=2, opts=None, transport="local", rows=1, switch_of=None, mode_of=None, fused16=None):
    """P ranks of a golden partitioning, a host thread each, epochs driven call by call (the Engine keeps one option value for a
    whole epoch; here the last layer's backward needs another).  The ranks meet at a barrier after every change of
    gatmh_bf16_gather: in-process peers read each other's value when an exchange starts.  Returns the downloads, the weights and
    the counters of every rank"""
    pobjs, parts = _golden(da, case)
    P, V = len(pobjs), len(parts)
    rng = np.random.default_rng(31)
    X = rng.uniform(-1, 1, (V, DIMS[0])).astype(np.float32)
    labels = rng.integers(0, DIMS[-1], V).astype(np.uint32)
    inw = [DIMS[0], ZW[0]]
    Ws = [(rng.standard_normal((inw[l], ZW[l])) / np.sqrt(inw[l])).astype(np.float32) for l in range(2)]
    Al = [(rng.standard_normal(ZW[l]) * 0.3).astype(np.float32) for l in range(2)]
    Ar = [(rng.standard_normal(ZW[l]) * 0.3).astype(np.float32) for l in range(2)]
    bar = threading.Barrier(P)
    box = {"msgs": [[[] for _ in range(P)] for _ in range(P)], "red": [None] * P}
    ctxs = []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, DIMS, V, r, P)
        ctx.gatmh_heads(HEADS)
        for k, v in dict({"spmm_blk_nb": 8, "local_timeout_ms": 5000}, **(opts or {})).items():
            ctx.set_option(k, v)
        part.upload(ctx, parts)
        ctx.preallocate()
        g = part.view()
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l in range(2):
            ctx.weight_set(l, "w", Ws[l]); ctx.weight_set(l, "a_l", Al[l]); ctx.weight_set(l, "a_r", Ar[l])
        ctx.adam_config(0.01)
        ctx.halo_fused_pack(fused)
        ctx.halo_fused_pack_bf16(fused if fused16 is None else fused16)
        ctx.gatmh_bwd_merged_exchange(merged)
        ctx.halo_bf16_rows(rows)
        ctx.gatmh_halo_bf16(switch if switch_of is None else switch_of[r])
        ctxs.append(ctx)
    if transport == "local":
        for c in ctxs:
            c.sync()
        da.Context.comm_init_local(ctxs)
    else:       # the scatter transport between the threads: every rank posts its messages, all meet, every rank takes its own
        def make(r):
            def exchange(msgs):
                for peer, m in msgs:
                    box["msgs"][peer][r].append(m.tobytes())
                bar.wait(30)
                mine = [m for s_ in range(P) for m in box["msgs"][r][s_]]
                if mine:
                    ctxs[r].scatter_msgs_deliver(mine)
                bar.wait(30)
                for s_ in range(P):
                    box["msgs"][r][s_] = []
                bar.wait(30)

            def allreduce(buf):
                box["red"][r] = buf.copy()
                bar.wait(30)
                total = box["red"][0].copy()
                for q in range(1, P):
                    total += box["red"][q]
                bar.wait(30)
                buf[:] = total
            return exchange, allreduce
        for r, c in enumerate(ctxs):
            c.set_scatter_transport(*make(r), 8192)
    errors = [None] * P

    def value(r, v):
        ctxs[r].set_option("gatmh_bf16_gather", v if mode_of is None else min(v, mode_of[r]))
        bar.wait(30)

    def rank(r):
        c = ctxs[r]
        try:
            for _ in range(epochs):
                value(r, MODE)
                for l in range(2):
                    c.apply_vertex(l, da.FORWARD)
                    c.halo_exchange(l + 1, da.FORWARD)
                    c.apply_edge(l + 1, da.FORWARD)
                    c.aggregate(l + 1, da.FORWARD)
                c.predict_gat(2)
                for l in (1, 0):
                    value(r, BWD_VALUE[l])
                    c.aggregate(l + 1, da.BACKWARD)
                    c.apply_vertex(l, da.BACKWARD)
                    c.weight_update(l)
            c.sync()
        except Exception as e:      # a failing rank must not leave the others waiting
            errors[r] = e
            bar.abort()

    th = [threading.Thread(target=rank, args=(r,)) for r in range(P)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    out = {"errors": errors, "views": _own_views(pobjs), "tensors": [], "weights": [], "wgrads": [], "kept": []}
    if not any(errors):
        for r, c in enumerate(ctxs):
            vw = out["views"][r]
            N, Gs, Gd = int(vw["localVtxCnt"]), int(vw["srcGhostCnt"]), int(vw["dstGhostCnt"])
            skip = lambda nm: (nm in ("fg_z", "fg_el") and not Gs) or (nm in ("bg_do", "bg_st") and not Gd)
            out["tensors"].append({(l, nm): c.download(l, nm) for (l, nm) in DL if not skip(nm)} if N else {})
            out["weights"].append([{nm: c.weight_get(l, nm) for nm in ("w", "a_l", "a_r")} for l in range(2)])
            out["wgrads"].append([{nm: c.weight_grad_get(l, nm) for nm in ("w", "a_l", "a_r")} for l in range(2)])
            out["kept"].append({"gat16": c.gatmh_halo_bf16_stats(), "bf16": c.halo_bf16_rows_stats(), "fused": c.halo_fused_pack_stats(),
                                "merged": c.gatmh_bwd_merged_exchange_stats()})
    for c in ctxs:
        c.sync()
    for c in ctxs:
        c.close()
    for p in pobjs:
        p.close()
    return out


def _equal(a, b, what):
    assert not any(a["errors"]) and not any(b["errors"]), (what, a["errors"], b["errors"])
    for r in range(len(a["tensors"])):
        assert set(a["tensors"][r]) == set(b["tensors"][r]), (what, r)
        for k in a["tensors"][r]:
            assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty"])
def test_epochs_over_the_local_transport(da, case):
    epochs = 2
    assert BWD_VALUE == [2, 1]
    on = _drive(da, case, 1, fused=1, merged=1)
    assert not any(on["errors"]), on["errors"]
    P = len(on["views"])
    # the ghost rows: fg_z the owner's z rounded, bg_st the owner's st; bg_do rounded where its layer ran with value 2
    _check_ghosts(on, [((l, "fg_z"), (l, "z"), "srcGhost", True) for l in range(2)] + [((l, "bg_st"), (l, "st"), "dstGhost", False) for l in range(2)] +
                  [((l, "bg_do"), (l, "do"), "dstGhost", BWD_VALUE[l] == 2) for l in range(2)], case)
    Gs = sum(int(len(g["srcGhost"])) for g in on["views"])
    Gd = sum(int(len(g["dstGhost"])) for g in on["views"])
    assert Gs > 0 and Gd > 0
    fwd_bytes = Gs * sum(2 * hb.row_elems(ZW[l], 0) for l in range(2))
    for fused in (0, 1):
        for merged in (0, 1):
            run = on if (fused, merged) == (1, 1) else _drive(da, case, 1, fused=fused, merged=merged)
            _equal(on, run, (case, "fused", fused, "merged", merged))
            row_b = 4 * gr.wire_row(ZW[0], HEADS[0], 0)[0] if merged else 2 * hb.row_elems(ZW[0], 0)
            assert sum(k["bf16"][1] for k in run["kept"]) == epochs * (fwd_bytes + Gd * row_b), (case, fused, merged, run["kept"])
            for r, k in enumerate(run["kept"]):
                assert k["gat16"][:2] == (2 * epochs, epochs), (case, fused, merged, r, k)          # z of both layers; do of layer 0
                assert k["gat16"][3] == (epochs if fused and merged and len(on["tensors"][r]) else 0) or not len(on["tensors"][r]), (case, r, k)
                assert k["merged"][0] == (2 * epochs if merged else 0), (case, fused, merged, r, k)
                if fused:       # every forward exchange took the rows the GEMM's bf16 epilogue wrote
                    assert k["fused"][0] >= 2 * epochs or not len(on["tensors"][r]), (case, fused, merged, r, k)
    _equal(on, _drive(da, case, 1, fused=1, merged=1, opts={"halo_overlap": 0}), (case, "halo_overlap 0"))
    _equal(on, _drive(da, case, 1, fused=1, merged=1, fused16=0), (case, "bf16 pack kernel in place of the send16 epilogue"))
    # against the switch off: fg_el comes from unrounded rows there, so the results move -- within the rounding's bound
    off = _drive(da, case, 0, fused=1, merged=1)
    assert not any(off["errors"]), off["errors"]
    for k in off["kept"]:
        assert k["gat16"] == (0, 0, 0, 0) and k["bf16"][:2] == (0, 0) and k["bf16"][2] > 0, k
    differ = 0
    for r in range(P):
        for l in range(2):
            if (l, "o") not in on["tensors"][r]:
                continue
            a, b, z = on["tensors"][r][(l, "o")], off["tensors"][r][(l, "o")], off["tensors"][r][(l, "z")]
            err, zmax = float(np.abs(a - b).max()), float(np.abs(z).max())
            differ += int(not np.array_equal(_bits(a), _bits(b)))
            print(f"\n{case} rank {r} layer {l}: max|o_on - o_off| = {err:.3e}, 2**-8 max|z| = {2.0 ** -8 * zmax:.3e}")
            if l in EL_TABLE_LAYERS[DIMS[1]]:
                assert err <= 2.0 ** -8 * zmax, (case, r, l, err, zmax)
    assert differ > 0, "fg_el moved: the results are not equal"


# ---- 4. not taken, ranks that disagree, refusals, inert cases ----------------------------------------------------------------------------
def test_direct_recv_plans_and_the_scatter_transport_keep_fp32(da):
    case = "parts_toy60_p2"
    for what, kw in (("halo_direct_recv = 1", dict(opts={"halo_direct_recv": 1})), ("scatter transport", dict(transport="scatter"))):
        off = _drive(da, case, 0, fused=1, merged=1, **kw)
        on = _drive(da, case, 1, fused=1, merged=1, **kw)
        _equal(off, on, what)
        for r in range(2):
            assert on["kept"][r]["gat16"] == (0, 0, 0, 0) and on["kept"][r]["bf16"][:2] == (0, 0), (what, r, on["kept"][r])
            assert on["kept"][r]["bf16"][2] == off["kept"][r]["bf16"][2] > 0, (what, r, on["kept"][r], off["kept"][r])
        # ... and the ghost rows are the owners' bits
        _check_ghosts(on, [((l, "fg_z"), (l, "z"), "srcGhost", False) for l in range(2)] + [((l, "bg_do"), (l, "do"), "dstGhost", False) for l in range(2)], what)


def test_local_ranks_that_disagree_fail_and_stay_usable(da):
    """the switch on rank 0 only: both ranks' first forward exchange fails with DORY_ERR_COMM; the gather value 2 on rank 0 and 1 on
    rank 1: the forward agrees (both ship bf16), the backward of the hidden layer fails.  The same contexts then run clean epochs"""
    case = "parts_toy60_p2"
    bad = _drive(da, case, 1, switch_of=[1, 0], epochs=1)
    assert all(e is not None for e in bad["errors"]), bad["errors"]
    assert any("error -4" in str(e) and "dory_halo_bf16_rows differs" in str(e) for e in bad["errors"]), bad["errors"]
    bad = _drive(da, case, 1, mode_of=[2, 1], epochs=1)
    assert any("error -4" in str(e) and "dory_halo_bf16_rows differs" in str(e) for e in bad["errors"]), bad["errors"]
    # one pair of contexts, stage by stage: refused, set right, then the exchange goes through
    pobjs, parts = _golden(da, case)
    ctxs = []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, DIMS, len(parts), r, 2)
        ctx.gatmh_heads(HEADS)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("local_timeout_ms", 300)
        ctx.set_option("gatmh_bf16_gather", 2)
        part.upload(ctx, parts)
        ctx.preallocate()
        g = part.view()
        ctx.fill_uniform(0, "h", 3, -1.0, 1.0, g["localToGlobal"])
        ctx.labels_upload(np.zeros(int(g["localVtxCnt"]), np.uint32))
        ctx.weights_init_xavier()
        ctx.halo_bf16_rows(1)
        ctx.gatmh_halo_bf16(1 - r)
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    for c in ctxs:
        c.apply_vertex(0, da.FORWARD)
    for r in (0, 1):
        with pytest.raises(da.DoryError, match=r"error -4.*dory_halo_bf16_rows differs.*dory_gatmh_halo_bf16"):
            ctxs[r].halo_exchange(1, da.FORWARD)
        assert ctxs[r].gatmh_halo_bf16_stats() == (0, 0, 0, 0) and ctxs[r].halo_bf16_rows_stats() == (0, 0, 0)
    ctxs[1].gatmh_halo_bf16(1)
    for c in ctxs:
        c.halo_exchange(1, da.FORWARD)
    for c in ctxs:
        c.apply_edge(1, da.FORWARD)
        c.aggregate(1, da.FORWARD)
        c.sync()
        assert c.gatmh_halo_bf16_stats() == (1, 0, 0, 0)
    for c in ctxs:
        c.close()
    for p in pobjs:
        p.close()


def test_refusals_and_the_single_partition(da):
    import aggregate_ref as ar
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_halo_bf16"):
        c.gatmh_halo_bf16(1)                                            # before dory_configure
    c.configure(da.GCN, [4, 41, 2], 100, 0, 2)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_halo_bf16.*DORY_GATMH"):
        c.gatmh_halo_bf16(1)                                            # a GCN context
    with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_wire_do"):
        c.gatmh_bwd_wire_do(0)
    c.close()
    c = da.Context(0)
    c.configure(da.GAT, [4, 16, 2], 100, 0, 2)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_halo_bf16.*DORY_GATMH"):
        c.gatmh_halo_bf16(1)                                            # the GAT prototype
    c.close()
    c = da.Context(0)
    c.configure(da.GATMH, [16, 32, 8], 100, 0, 2)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="error -1.*gatmh_halo_bf16"):
            c.gatmh_halo_bf16(bad)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_bwd_wire_do.*dory_preallocate"):
        c.gatmh_bwd_wire_do(0)
    c.gatmh_halo_bf16(1)                                                # any time after dory_configure
    c.gatmh_halo_bf16(0)
    assert c.gatmh_halo_bf16_stats() == (0, 0, 0, 0)
    c.close()
    # a single partition: accepted and inert; refused while an epoch graph is being recorded
    g = ar.graph("uniform:200:1500")
    rng = np.random.default_rng(4)
    X = rng.uniform(-1, 1, (200, 16)).astype(np.float32)
    labels = rng.integers(0, 8, 200).astype(np.uint32)
    runs = []
    for on in (0, 1):
        one = da.Context(0)
        one.configure(da.GATMH, [16, 32, 8], 200)
        one.gatmh_heads([4, 2])
        one.set_option("spmm_blk_nb", 8)
        one.set_option("gatmh_bf16_gather", 2)
        one.graph_upload(g)
        one.preallocate()
        one.upload(0, "h", X)
        one.labels_upload(labels)
        wr = np.random.default_rng(8)
        for l, (fi, fo) in enumerate(((16, 32), (32, 16))):
            one.weight_set(l, "w", (wr.standard_normal((fi, fo)) / np.sqrt(fi)).astype(np.float32))
            one.weight_set(l, "a_l", (wr.standard_normal(fo) * 0.3).astype(np.float32))
            one.weight_set(l, "a_r", (wr.standard_normal(fo) * 0.3).astype(np.float32))
        one.halo_bf16_rows(on)
        one.gatmh_halo_bf16(on)
        one.adam_config(0.01)
        eng = da.NativeEngine(one)
        eng.run(1)
        one.sync()
        assert one.gatmh_halo_bf16_stats() == (0, 0, 0, 0) and one.halo_bf16_rows_stats() == (0, 0, 0)
        runs.append({"t": {(l, nm): _bits(one.download(l, nm)) for l in range(2) for nm in ("z", "o", "t", "der", "del", "dz")},
                     "W": [_bits(one.weight_get(l, nm)) for l in range(2) for nm in ("w", "a_l", "a_r")]})
        eng.close()
        if on:
            one.epoch_graph_begin()
            with pytest.raises(da.DoryError, match="error -1.*epoch graph is being recorded"):
                one.gatmh_halo_bf16(0)
            one.epoch_graph_drop()
            one.gatmh_halo_bf16(0)
        one.close()
    for k in runs[0]["t"]:
        assert np.array_equal(runs[0]["t"][k], runs[1]["t"][k]), k
    for a, b in zip(runs[0]["W"], runs[1]["W"]):
        assert np.array_equal(a, b)


# ---- 5. replay ------------------------------------------------------------------------------------------------------------------------------
def test_replayed_epochs_with_all_switches_on_equal_eager_epochs(da):
    """an epoch graph records a single partition only (the exchange is not recorded): with every switch of the halo path on, an
    epoch recorded after one eager epoch replays bit for bit what eager epochs compute"""
    import partition_oracle as po
    V, E, dims, heads = 600, 2400, [24, 32, 8], [4, 2]
    states = []
    for graph in (0, 1):
        rng = np.random.default_rng(5)
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        g = po.preprocess(np.concatenate([s, d]), np.concatenate([d, s]), np.zeros(V, np.int64), 0, 1)
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.fill_uniform(0, "h", 3, -1.0, 1.0, g["localToGlobal"])
        ctx.labels_upload(rng.integers(0, 8, V).astype(np.uint32))
        ctx.weights_init_xavier()
        ctx.adam_config(0.01)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.halo_fused_pack(1)
        ctx.halo_fused_pack_bf16(1)
        ctx.gatmh_bwd_merged_exchange(1)
        ctx.halo_bf16_rows(1)
        ctx.gatmh_halo_bf16(1)
        ctx.set_option("epoch_graph", graph)
        eng = da.NativeEngine(ctx)
        eng.run(4)
        if graph:
            assert ctx.get_option("epoch_graph_recorded") == 1
        assert ctx.gatmh_halo_bf16_stats() == (0, 0, 0, 0)
        st = {}
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                st[(nm, l)] = ctx.weight_get(l, nm)
                st[("d" + nm, l)] = ctx.weight_grad_get(l, nm)
            for nm in ("z", "o", "op", "dz", "el", "t", "del"):
                st[(nm, l)] = ctx.download(l, nm)
        states.append(st)
        eng.close()
        ctx.close()
    for k in states[0]:
        assert np.array_equal(_bits(states[0][k]), _bits(states[1][k])), k
