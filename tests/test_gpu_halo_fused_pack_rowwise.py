"""dory_halo_fused_pack_rowwise (include/dorylus_hip.h): with dory_halo_fused_pack on, the row-wise kernels that produce the source
of an exchange -- tanh_backward (g of a transform-first layer), softmax + loss (g of a transform-first last layer), tanh_forward (h
of a transform-first layer) and the GAT prototype's softmax - label (its last layer's grad) -- run their send forms
(csrc/elementwise.hip: tanh_backward_send_kernel, tanh_forward_send_kernel, softmax_rows_send_kernel) and the exchange runs no
pack kernel.  Every comparison is bit for bit.

  1. stage level: one context as rank 0 of 4 with a host transport that records what travels; the bytes are what dory_halo_pack
     (the pack kernel the wire rule picks) writes for the tensor as it is, in the fp32 padded, fp32 exact and bf16 wire formats; the
     produced tensor keeps the bits of the same call with the switch off; the counters; a second exchange is a fallback; a
     one-column tensor under a bf16 wire packs;
  2. every way the stamp can go stale between producer and exchange, and a producer that runs again with the switch off;
  3. epochs over the in-process transport and over the host transport in two processes, the new switch off against on: the same
     bits everywhere, and no exchange of the transform-first orders and of the GAT prototype packs any more; the multi-head GAT's
     do / st still do;
  4. refused arguments, the single partition."""
import os
import sys
import traceback

import numpy as np
import pytest

from test_gpu_halo_fused_pack import _bits, _graph, _send_lists

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4
MS = (1, 31, 129, 300)
TANH_COLS = (7, 32, 41, 64, 65, 128, 130)
SOFTMAX_COLS = (2, 8, 9, 16, 17, 32, 33, 41, 48, 49, 64, 65, 130)     # every lanes-per-row branch, one and several columns a lane
GUARD = 64


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _pad_ld(cols):
    return cols if cols <= 1 else (cols + 31) // 32 * 32


def _cases():
    out = []
    for forms, widths in ((("g_tanh", "h_tanh"), TANH_COLS), (("g_xent", "grad_gat"), SOFTMAX_COLS)):
        for fi, form in enumerate(forms):
            for i, cols in enumerate(widths):
                out.append((MS[(i + fi) % len(MS)], cols, form))
    for form in ("g_tanh", "h_tanh", "g_xent", "grad_gat"):                   # every form at every M
        assert {m for m, _, f in out if f == form} == set(MS), form
    return out


CASES = _cases()


class Rig:
    """one context, rank 0 of 4, whose host transport records what every exchange sends; `form` names the row-wise producer"""

    def __init__(self, da, M, cols, form, variant=0, both_dirs=False):
        import torch
        from helpers import make_ctx
        self.da, self.M, self.cols, self.form, self.torch = da, M, cols, form, torch
        gnn, opts = da.GCN, {"gcn_transform_first": 2}
        if form == "g_tanh":       # g@0 = aTg@0 * (1 - tanh(z@0)^2) of a transform-first layer, sent backward into bgg@0
            dims, self.src, self.xl, self.xdir = [cols + 3, cols, 2], (0, "g"), 0, da.BACKWARD
            self.inputs, self.call = [(0, "aTg"), (0, "z")], lambda c: c.apply_vertex(0, da.BACKWARD)
        elif form == "g_xent":     # g@1 = (softmax(z@1) - lab) / n of a transform-first last layer, sent backward into bgg@1
            dims, self.src, self.xl, self.xdir = [cols + 5, cols + 3, cols], (1, "g"), 1, da.BACKWARD
            self.inputs, self.call = [(1, "z")], lambda c: c.apply_vertex(1, da.FORWARD)
        elif form == "h_tanh":     # h@0 = tanh(z@0) of the one transform-first layer, sent forward into fg@1
            opts = {"gcn_transform_first": 1}
            dims, self.src, self.xl, self.xdir = [cols + 3, cols, 2], (0, "h"), 1, da.FORWARD
            self.inputs, self.call = [(0, "z")], lambda c: c.apply_vertex(0, da.FORWARD)
        else:                      # grad_gat: grad@1 = softmax(ah@1) - lab of the GAT prototype, sent backward into bg_d@1
            gnn, opts = da.GAT, {}
            dims, self.src, self.xl, self.xdir = [4, 5, cols], (1, "grad"), 2, da.BACKWARD
            self.inputs, self.call = [(1, "ah")], lambda c: c.predict_gat(2)
        self.dims, self.gnn = dims, gnn
        ctx = self.ctx = make_ctx(da, _graph(M), dims, 4 * M + 8, gnn=gnn, node_id=0, num_nodes=P, options=opts)
        if form in ("g_tanh", "h_tanh"):
            assert ctx.transform_first_layer(0)
        if form == "g_xent":
            assert ctx.transform_first_layer(1)
        if form == "h_tanh":
            assert not ctx.transform_first_layer(1)
        self.lists = _send_lists(M, variant)
        self.total = sum(len(l) for l in self.lists)
        self.plan(self.xdir)
        if both_dirs:
            self.plan(1 - self.xdir)
        ctx.labels_upload(np.random.default_rng([2, M, cols]).integers(0, dims[-1], M).astype(np.uint32))
        self.new_input(0)
        self.sent = []

        def alltoallv(send, sc, so, recv, rc, ro):
            n = int((so + sc).max())
            self.sent.append((np.array(send[:n], copy=True), [int(x) for x in sc], [int(x) for x in so]))
        ctx.set_host_transport(alltoallv, lambda buf: None)
        self.cap = (max(1, sum(len(l) for l in _send_lists(M, 0))) + 8) * max(4, _pad_ld(cols)) * 4
        self.rows_on = False

    def plan(self, direction):
        self.ctx.halo_plan(direction, self.lists, [[], [2], [0], [1]])

    def new_input(self, salt):
        for layer, name in self.inputs:
            rng = np.random.default_rng([5, self.M, self.cols, salt, len(name)])
            self.ctx.upload(layer, name, rng.uniform(-2, 2, (self.M, self.cols)).astype(np.float32))

    def produce(self):
        self.call(self.ctx)

    def bf16_wire(self, on):
        """every switch a bf16 wire of this exchange needs (but dory_halo_fused_pack itself)"""
        if self.gnn == self.da.GAT:
            self.ctx.gat_bf16_gather(2 if on else 0)
        else:
            self.ctx.set_option("gcn_bf16_gather", 2 if on else 0)
        self.ctx.halo_bf16_rows(int(on))
        self.ctx.halo_fused_pack_bf16(int(on))
        self.rows_on = bool(on)

    def counters(self):
        c = self.ctx
        return {"fused": np.array(c.halo_fused_pack_stats(), np.int64), "rw": np.array(c.halo_fused_pack_rowwise_stats(), np.int64),
                "f16": np.array(c.halo_fused_pack_bf16_stats(), np.int64), "bf16": np.array(c.halo_bf16_rows_stats(), np.int64),
                "packed": np.array([int(c.get_option("halo_rows_packed")), int(c.get_option("halo_floats_packed"))], np.int64)}

    def wire(self):
        return self.ctx.halo_wire_row(self.xl, self.xdir)

    def kernel_pack(self):
        """dory_halo_pack of the exchange into a guarded device buffer: the bytes of the pack kernel the wire rule picks"""
        eb, re = self.wire()
        n = self.total * re * eb
        assert n <= self.cap
        buf = self.torch.full((self.cap + GUARD,), 0x5A, dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        self.ctx.halo_pack(self.xl, self.xdir, buf.data_ptr())
        self.ctx.sync()
        got = buf.cpu().numpy()
        assert (got[n:] == 0x5A).all(), "the reference pack wrote behind its rows"
        return got[:n].copy()

    def exchange(self):
        n = len(self.sent)
        self.ctx.halo_exchange(self.xl, self.xdir)
        self.ctx.sync()
        assert len(self.sent) == n + 1
        return self.sent[-1]

    def check(self, path, what):
        """one exchange: the current tensor's rows travel in the current wire format, laid out as the pack kernel lays them out;
        `path`: "fused16" / "fused32" (a row-wise producer wrote them: no pack kernel), "pack16" / "pack32" (a counted fallback),
        "off16" / "off32" (dory_halo_fused_pack off: a pack, nothing counted by the fused pack)"""
        eb, re = self.wire()
        assert eb == (2 if path.endswith("16") else 4), (what, path, eb)
        if eb == 4:
            assert re == (self.cols if self.ctx.get_option("halo_exact_rows") else _pad_ld(self.cols)), (what, re)
        want = self.kernel_pack()
        before = self.counters()
        send, sc, so = self.exchange()
        fl = re * eb // 4
        assert sc == [len(l) * fl for l in self.lists], (what, sc)
        assert so == [int(x) * fl for x in np.cumsum([0] + [len(l) for l in self.lists[:-1]])], (what, so)
        got = np.ascontiguousarray(send, np.float32).view(np.uint8)
        assert got.size == want.size == self.total * re * eb, (what, got.size, want.size)
        assert np.array_equal(got, want), (what, path, "bytes on the wire", int((got != want).sum()))
        T, nbytes, kind = self.total, self.total * re * eb, path[:-2]
        d = {k: (v - before[k]).tolist() for k, v in self.counters().items()}
        want_d = {
            "fused": [1, T, 0] if kind == "fused" else [0, 0, 1] if kind == "pack" else [0, 0, 0],
            "rw": [1, T] if kind == "fused" else [0, 0],
            "f16": [1, T] if path == "fused16" else [0, 0],
            "bf16": [1, nbytes, 0] if eb == 2 else [0, 0, int(self.rows_on)],
            "packed": [0, 0] if kind == "fused" else [T, T * fl],
        }
        assert d == want_d, (what, path, d, want_d)
        return got


def _stage(da, M, cols, form, variant):
    rig = Rig(da, M, cols, form, variant)
    ctx = rig.ctx
    assert ctx.halo_fused_pack_rowwise_stats() == (0, 0)
    rig.produce()                                                  # every switch off: the reference bits of the tensor
    ref = _bits(ctx.download(*rig.src))
    assert np.isfinite(ctx.download(*rig.src)).all() and ref.any()
    ctx.halo_fused_pack(1)
    rig.produce()
    rig.check("pack32", (variant, "the new switch off: a fallback, as before it existed"))
    ctx.halo_fused_pack_rowwise(1)
    for bf16 in (0, 1):
        rig.bf16_wire(bf16)
        sfx = "16" if bf16 else "32"
        for exact in (0, 1):
            ctx.set_option("halo_exact_rows", exact)
            what = (variant, bf16, exact)
            rig.produce()
            rig.check("fused" + sfx, what + ("fused",))          # (the reference pack in between left the stamp alone)
            assert np.array_equal(_bits(ctx.download(*rig.src)), ref), what + ("the tensor's bits",)
            rig.check("pack" + sfx, what + ("second exchange of the same rows: the stamp was consumed",))
    ctx.close()


@pytest.mark.parametrize("M,cols,form", CASES, ids=[f"M{m}-c{c}-{f}" for m, c, f in CASES])
def test_send_forms_write_the_pack_kernels_bytes(da, M, cols, form):
    for variant in ((0, 1) if (M + cols) % 2 else (0,)):              # the plan with an empty peer: every other case
        _stage(da, M, cols, form, variant)


@pytest.mark.parametrize("form", ["g_tanh", "h_tanh"])
def test_grid_stride_loops_take_a_second_turn(da, form):
    """40 000 x 128: 1.28 M quads, more than the 4096 (tanh_backward) / 8192 (tanh_forward) workgroups of 256 lanes hold at once"""
    _stage(da, 40000, 128, form, 0)


@pytest.mark.parametrize("form", ["g_xent", "grad_gat"])
def test_one_column_tensor_is_a_counted_fallback(da, form):
    """ld == 1: a bf16 wire row of 4 elements is wider than the tensor's row, so no producer may write it -- a counted fallback with
    the right bytes, as for the GEMMs.  (Its fp32 rows have no pack kernel at all -- 16-byte lanes -- so only the bf16 wire ships it.)"""
    rig = Rig(da, 31, 1, form)
    ctx = rig.ctx
    rig.produce()
    ref = _bits(ctx.download(*rig.src))
    ctx.halo_fused_pack(1)
    ctx.halo_fused_pack_rowwise(1)
    rig.bf16_wire(1)
    for exact in (0, 1):
        ctx.set_option("halo_exact_rows", exact)
        assert rig.wire() == (2, 4)
        rig.produce()
        rig.check("pack16", ("one column, bf16", exact))
        assert np.array_equal(_bits(ctx.download(*rig.src)), ref)
    ctx.close()


# ---- 2. stale stamps --------------------------------------------------------------------------------------------------------------
def test_stale_stamps_fall_back(da):
    rig = Rig(da, 129, 41, "g_tanh", both_dirs=True)
    ctx = rig.ctx
    ctx.halo_fused_pack(1)
    ctx.halo_fused_pack_rowwise(1)
    rig.produce()
    rig.check("fused32", "nothing in between")
    # the producer twice: the second call's rows, fused
    rig.produce()
    rig.new_input(1)
    rig.produce()
    rig.check("fused32", "produced twice")
    # an upload of g between producer and exchange: the new rows travel, packed by the kernel
    rig.produce()
    new = np.random.default_rng(1).uniform(-1, 1, (129, 41)).astype(np.float32)
    ctx.upload(0, "g", new)
    got = rig.check("pack32", "dory_tensor_upload in between")
    assert np.array_equal(got.view(np.uint32).reshape(rig.total, -1)[:, :41], _bits(new[np.concatenate(rig.lists).astype(np.int64)]))
    # dory_tensor_fill_uniform likewise
    rig.produce()
    ctx.fill_uniform(0, "g", 99)
    rig.check("pack32", "dory_tensor_fill_uniform in between")
    # an upload of ANOTHER tensor leaves the stamp alone
    rig.produce()
    ctx.upload(0, "h", np.zeros((129, 41), np.float32))
    rig.check("fused32", "an upload of another tensor")
    # another exchange packs into the internal buffer in between
    rig.produce()
    before = rig.counters()["fused"]
    ctx.halo_exchange(1, da.FORWARD)                               # xw@1: nobody produced it
    rig.check("pack32", "another exchange in between")
    assert (rig.counters()["fused"] - before).tolist() == [0, 0, 2]
    # the new switch off and on again
    rig.produce()
    ctx.halo_fused_pack_rowwise(0)
    ctx.halo_fused_pack_rowwise(1)
    rig.check("pack32", "dory_halo_fused_pack_rowwise off and on in between")
    # ... and dory_halo_fused_pack
    rig.produce()
    ctx.halo_fused_pack(0)
    rig.check("off32", "dory_halo_fused_pack(0) in between")
    ctx.halo_fused_pack(1)
    rig.check("pack32", "on again, nothing produced since")
    # g can carry a stamp now: fused once, the switch off, the producer again on new inputs -- the second call's rows travel
    rig.produce()
    first = _bits(ctx.download(0, "g")).copy()
    ctx.halo_fused_pack_rowwise(0)
    rig.new_input(2)
    rig.produce()                                                  # the plain kernel rewrites g
    assert not np.array_equal(_bits(ctx.download(0, "g")), first)
    rig.check("pack32", "the producer again with the switch off")
    ctx.halo_fused_pack_rowwise(1)
    # the wire turns bf16 between producer and exchange, and back
    rig.produce()
    rig.bf16_wire(1)
    rig.check("pack16", "a bf16 wire in between")
    rig.produce()
    rig.check("fused16", "bf16 rows")
    rig.produce()
    ctx.halo_fused_pack_bf16(0)
    rig.check("pack16", "dory_halo_fused_pack_bf16(0) in between")
    rig.produce()
    rig.check("pack16", "a bf16 wire without dory_halo_fused_pack_bf16: the producer does not write it")
    rig.bf16_wire(0)
    # a new plan in between (other lists: the slots move)
    rig.produce()
    rig.lists = _send_lists(129, 1)
    rig.total = sum(len(l) for l in rig.lists)
    rig.plan(da.BACKWARD)
    rig.check("pack32", "dory_halo_plan in between")
    rig.produce()
    rig.check("fused32", "the new plan's map")
    # halo_exact_rows changed: 64 floats a row in the buffer, 41 on the wire
    rig.produce()
    ctx.set_option("halo_exact_rows", 1)
    rig.check("pack32", "halo_exact_rows changed in between")
    rig.produce()
    rig.check("fused32", "exact rows")
    # the raw pointer handed out: this tensor packs from now on, whatever is produced
    rig.produce()
    assert ctx.info(0, "g")[3]
    rig.check("pack32", "raw pointer handed out after the producer")
    rig.produce()
    rig.check("pack32", "raw pointer: sticky")
    ctx.close()


@pytest.mark.parametrize("form", ["g_tanh", "g_xent"])
def test_an_unfused_producer_drops_the_stamp_of_g(da, form):
    """the note the two producers of g leave when they run their plain kernels.  The setter of the new switch drops the stamp itself,
    so this goes by a route that does not: the producer stamps g under an fp32 wire; option gcn_bf16_gather turns the wire bf16
    (the stamp stays, as tests/test_gpu_halo_fused_pack_bf16.py pins); the producer runs again on new inputs and, without
    dory_halo_fused_pack_bf16, runs its plain kernel; the option turns the wire fp32 again.  Source, direction, width, kind and
    buffer of the stamp would all match the exchange: only the producer's own note keeps the first call's rows off the wire."""
    rig = Rig(da, 129, 41, form)
    ctx = rig.ctx
    ctx.halo_fused_pack(1)
    ctx.halo_fused_pack_rowwise(1)
    ctx.halo_bf16_rows(1)
    rig.rows_on = True
    rig.produce()                                                  # fp32 rows of the first inputs in the buffer, g stamped
    first = _bits(ctx.download(*rig.src)).copy()
    ctx.set_option("gcn_bf16_gather", 2)
    ctx.set_option("gcn_bf16_gather", 0)
    rig.check("fused32", (form, "the option there and back leaves the stamp alone"))
    rig.produce()
    ctx.set_option("gcn_bf16_gather", 2)
    assert rig.wire()[0] == 2
    rig.new_input(3)
    rig.produce()                                                  # a bf16 wire nobody fuses: the plain kernel writes g
    assert not np.array_equal(_bits(ctx.download(*rig.src)), first)
    ctx.set_option("gcn_bf16_gather", 0)
    rig.check("pack32", (form, "the second call's rows"))
    ctx.close()


# ---- 3. epochs ------------------------------------------------------------------------------------------------------------------------
def _golden(da, name):
    import glob
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


def _directed_parts(da, Pn=2, seed=17, V=240, E=2600):
    """partitions built from directed records: the golden ones carry symmetrised edge values, with which the library keeps the
    aggregate-first order whatever the option says"""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % Pn).astype(np.int32)
    return lambda: ([da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, Pn) for r in range(Pn)], parts)


def _same_bits(a, b, what):
    for r in range(len(a["tensors"])):
        assert set(a["tensors"][r]) == set(b["tensors"][r]), (what, r)
        for k in a["tensors"][r]:
            assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(len(a["weights"][r])):
            for nm in a["weights"][r][l]:
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


def _run(da, gnn, case, dims, epochs, opts, on, dl, bf16=False, heads=None, seed=5):
    """one run_local with dory_halo_fused_pack on and the new switch as asked (bf16: with gather mode 2, bf16 rows, twins and the
    fused pack's bf16 form); returns (run_local's result, {rank: counters just before the context closes})"""
    from local_ranks import run_local
    pobjs, parts = case() if callable(case) else _golden(da, case)
    V, L = len(parts), len(dims) - 1
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    zw = [dims[l + 1] * (heads[l] if heads and l == L - 1 else 1) for l in range(L)]      # (multi-head: hidden widths hold all heads)
    inw = [dims[0]] + zw[:-1]
    Ws = [(rng.standard_normal((inw[l], zw[l])) / np.sqrt(inw[l])).astype(np.float32) for l in range(L)]
    As = [(rng.standard_normal((dims[l + 1], 1)) / 2).astype(np.float32) for l in range(L)]
    Al = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
    Ar = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
    kept = {}

    def setup(ctx, r, g):
        if g["localVtxCnt"]:
            ctx.upload(0, "x" if gnn == da.GCN else "h", X[g["localToGlobal"]])
        if gnn == da.GCN and g["srcGhostCnt"]:
            ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), dims[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l in range(L):
            ctx.weight_set(l, "w", Ws[l])
            if gnn == da.GAT:
                ctx.weight_set(l, "a_i", As[l])
            elif gnn == da.GATMH:
                ctx.weight_set(l, "a_l", Al[l])
                ctx.weight_set(l, "a_r", Ar[l])
        if gnn == da.GAT and bf16:
            ctx.gat_bf16_gather(2)
        ctx.halo_fused_pack(1)
        if bf16:
            ctx.halo_bf16_rows(1)
            ctx.halo_bf16_ghosts(1)
            ctx.halo_fused_pack_bf16(1)
        ctx.halo_fused_pack_rowwise(on)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"fused": ctx.halo_fused_pack_stats(), "rw": ctx.halo_fused_pack_rowwise_stats(),
                           "f16": ctx.halo_fused_pack_bf16_stats(), "bf16": ctx.halo_bf16_rows_stats(),
                           "packed": int(ctx.get_option("halo_rows_packed")),
                           "made": int(ctx.get_option("halo_direct_recvs")) + int(ctx.get_option("halo_staged_recvs")),
                           "tf": [ctx.transform_first_layer(l) for l in range(L)] if gnn == da.GCN else []}
            close()
        ctx.close = closing
    if gnn == da.GCN and bf16:
        opts = dict(opts, gcn_bf16_gather=2)
    out = run_local(da, pobjs, parts, dims, gnn, epochs, setup, opts, downloads=dl,
                    pre=(lambda c: c.gatmh_heads(heads)) if heads else None, wnames=("w", "a_l", "a_r") if heads else None)
    return out, kept


def _off_on(da, gnn, case, dims, epochs, opts, dl, what, **kw):
    """the configuration against itself, only the new switch differing: the same bits, the same exchanges made, what travelled as
    bf16 counted the same; with the switch off nothing counts in the new counters"""
    off, koff = _run(da, gnn, case, dims, epochs, opts, 0, dl, **kw)
    on, kon = _run(da, gnn, case, dims, epochs, opts, 1, dl, **kw)
    _same_bits(off, on, what)
    assert set(koff) == set(kon)
    for r in koff:
        assert koff[r]["rw"] == (0, 0), (what, r, koff[r])
        assert koff[r]["made"] == kon[r]["made"] and koff[r]["bf16"] == kon[r]["bf16"], (what, r, koff[r], kon[r])
        for k in (koff[r], kon[r]):
            assert k["fused"][0] + k["fused"][2] == k["made"], (what, r, k)
        # what the new switch takes is exactly what fell back without it, and nothing else moves
        assert kon[r]["rw"][0] == kon[r]["fused"][0] - koff[r]["fused"][0] == koff[r]["fused"][2] - kon[r]["fused"][2], (what, r, koff[r], kon[r])
        assert kon[r]["rw"][1] == kon[r]["fused"][1] - koff[r]["fused"][1], (what, r, koff[r], kon[r])
    return on, koff, kon


def _gcn_dl(L, tf):
    dl = [(l, "z") for l in range(L)] + [(l, nm) for l in range(L - 1) for nm in ("h", "aTg")]
    if tf:
        return dl + [(l, "g") for l in range(L)] + [(l, "bgg") for l in range(L)] + [(l, nm) for l in range(1, L) for nm in ("xw", "fgxw")]
    return dl + [(l, "ah") for l in range(L)] + [(l, nm) for l in range(1, L) for nm in ("grad", "fg")] + [(l, "bg") for l in range(L - 1)]


def _all_fused(on, kon, what):
    for r, vw in enumerate(on["views"]):
        if int(vw["localVtxCnt"]):
            assert kon[r]["fused"][2] == 0 and kon[r]["fused"][0] == kon[r]["made"] > 0, (what, r, kon[r])


TF_CASES = {"random_p2": lambda da: _directed_parts(da, 2, 17), "random_p3": lambda da: _directed_parts(da, 3, 23),
            "parts_toy60_p4_hash": lambda da: "parts_toy60_p4_hash"}


@pytest.mark.parametrize("case", sorted(TF_CASES))
def test_gcn_transform_first_every_exchange_fused(da, case):
    """33-25-6-3 with gcn_transform_first = 2: xw@1, xw@2 forward (GEMM outputs), g@2 (softmax + loss), g@1, g@0 (tanh backward)
    backward -- with the switch on no exchange packs.  (The golden partition carries symmetrised edge values: the library keeps the
    aggregate-first order there, whose exchanges the GEMMs cover alone.)"""
    dims, epochs = [33, 25, 6, 3], 2
    for exact in (0, 1):
        what = (case, exact)
        opts = {"spmm_blk_nb": 8, "gcn_transform_first": 2, "halo_exact_rows": exact}
        tf = not case.startswith("parts_")
        on, koff, kon = _off_on(da, da.GCN, TF_CASES[case](da), dims, epochs, opts, _gcn_dl(3, tf), what)
        _all_fused(on, kon, what)
        for r in kon:
            assert kon[r]["tf"] == [tf] * 3, (what, r, kon[r])
            if tf:
                assert kon[r]["rw"][0] == epochs * 3 and kon[r]["fused"][0] == epochs * 5, (what, r, kon[r])
            else:
                assert kon[r]["rw"] == (0, 0), (what, r, kon[r])


def test_gcn_transform_first_layer_0_only(da):
    """33-25-6 with gcn_transform_first = 1: h@0 (tanh forward) travels forward, grad@1 (a GEMM output) and g@0 (tanh backward)
    backward"""
    dims, epochs = [33, 25, 6], 2
    for exact in (0, 1):
        what = ("layer 0 only", exact)
        opts = {"spmm_blk_nb": 8, "gcn_transform_first": 1, "halo_exact_rows": exact}
        dl = [(0, "z"), (1, "z"), (0, "h"), (0, "aTg"), (0, "g"), (1, "g"), (1, "grad"), (1, "fg"), (0, "bg"), (0, "bgg"), (1, "ah")]
        on, koff, kon = _off_on(da, da.GCN, _directed_parts(da), dims, epochs, opts, dl, what)
        _all_fused(on, kon, what)
        for r in kon:
            assert kon[r]["tf"] == [True, False] and kon[r]["rw"][0] == epochs * 2 and kon[r]["fused"][0] == epochs * 3, (what, r, kon[r])


def test_gat_prototype_epoch(da):
    """z@0, z@1 forward and grad@0 backward are GEMM outputs, the last layer's grad comes from the softmax: four fused exchanges"""
    dims, L = [20, 16, 6], 2
    dl = [(l, nm) for l in range(L) for nm in ("z", "ah", "grad", "aTg", "fg_z", "bg_d")]
    for exact in (0, 1):
        what = ("GAT prototype", exact)
        on, koff, kon = _off_on(da, da.GAT, "parts_toy60_p2", dims, 1, {"spmm_blk_nb": 8, "halo_exact_rows": exact}, dl, what, seed=11)
        for r in kon:
            assert kon[r]["fused"][0] == 4 and kon[r]["fused"][2] == 0 and kon[r]["rw"][0] == 1, (what, r, kon[r])
            assert koff[r]["fused"][0] == 3 and koff[r]["fused"][2] == 1, (what, r, koff[r])
    on, koff, kon = _off_on(da, da.GAT, "parts_toy60_p2", dims, 1, {"spmm_blk_nb": 8}, dl, "GAT prototype, bf16", seed=11, bf16=True)
    for r in kon:
        assert kon[r]["fused"][0] == 4 and kon[r]["fused"][2] == 0 and kon[r]["rw"][0] == 1 and kon[r]["f16"][0] == 4, ("bf16", r, kon[r])


def test_gcn_transform_first_every_bf16_switch_on(da):
    """the first configuration under gather mode 2 with bf16 rows, twins and the fused pack's bf16 form: every exchange ships bf16
    rows its producer wrote, and the new counters count the g exchanges"""
    dims, epochs = [33, 25, 6, 3], 2
    for exact in (0, 1):
        what = ("every bf16 switch", exact)
        opts = {"spmm_blk_nb": 8, "gcn_transform_first": 2, "halo_exact_rows": exact}
        on, koff, kon = _off_on(da, da.GCN, _directed_parts(da), dims, epochs, opts, _gcn_dl(3, True), what, bf16=True)
        _all_fused(on, kon, what)
        for r in kon:
            assert kon[r]["rw"][0] == epochs * 3 and kon[r]["f16"][0] == epochs * 5 == kon[r]["bf16"][0], (what, r, kon[r])
            assert koff[r]["f16"][0] == epochs * 2 and koff[r]["fused"][2] == epochs * 3, (what, r, koff[r])


def test_gat_mh_do_st_still_pack(da):
    """the 8-head GAT: z@0 and z@1 forward fused as ever; do / st of both layers' backward sweeps -- two exchanges in a row through
    one send buffer, which halo_route never names -- keep packing, and its grad (dory_predict_gat) travels nowhere"""
    dims, heads = [40, 128, 41], [8, 1]
    dl = [(l, nm) for l in range(2) for nm in ("z", "o", "t", "del", "der", "dz", "fg_z", "bg_do", "bg_st")] + [(1, "logits")]
    on, koff, kon = _off_on(da, da.GATMH, _directed_parts(da), dims, 1, {"spmm_blk_nb": 8}, dl, "8-head GAT", heads=heads, seed=18)
    for r in kon:
        assert kon[r]["fused"] == koff[r]["fused"] and kon[r]["fused"][0] == 2 and kon[r]["rw"] == (0, 0), (r, kon[r], koff[r])
        assert kon[r]["packed"] == koff[r]["packed"] > 0, (r, kon[r], koff[r])       # (the rows the pack kernels moved: do / st among them)


# ---- the host transport: two processes on one GPU (worker pattern of tests/test_gpu_halo_fused_pack.py) -----------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


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
        dims, epochs = [33, 25, 6, 3], 2
        pobjs, parts = _directed_parts(da)()
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

        def run(on):
            ctx = da.Context(0)
            ctx.configure(da.GCN, dims, V, rank, world)
            for k, v in (("spmm_blk_nb", 8), ("gcn_transform_first", 2)):
                ctx.set_option(k, v)
            ctx.halo_fused_pack(1)             # before the plans: dory_halo_plan builds the maps
            ctx.halo_fused_pack_rowwise(on)
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
            ctx.set_host_transport(alltoallv, allreduce)
            assert all(ctx.transform_first_layer(l) for l in range(L))
            eng = da.NativeEngine(ctx)
            eng.run(epochs)
            ctx.sync()
            res = {"seen": seen, "fused": ctx.halo_fused_pack_stats(), "rw": ctx.halo_fused_pack_rowwise_stats(), "tensors": {}, "W": [], "dW": []}
            for l, nm in [(l, nm) for l in range(L) for nm in ("z", "g", "bgg")] + [(0, "h"), (1, "h"), (1, "xw"), (2, "xw"), (1, "fgxw"), (2, "fgxw")]:
                if ctx.info(l, nm, ptr=False)[0]:
                    res["tensors"][(l, nm)] = ctx.download(l, nm)
            for l in range(L):
                res["W"].append(ctx.weight_get(l))
                res["dW"].append(ctx.weight_grad_get(l))
            eng.close()
            ctx.close()
            return res
        out = {on: run(on) for on in (0, 1)}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_host_transport_two_processes_same_bits():
    """two processes on one GPU, the bytes over gloo, two transform-first epochs: the same counts, offsets and bits as with the new
    switch off, and no exchange packs"""
    import torch.multiprocessing as mp
    world, epochs = 2, 2
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
    for rank, r in res:
        off, on = r[0], r[1]
        assert set(off["tensors"]) == set(on["tensors"]) and len(on["tensors"]) >= 9
        for k in off["tensors"]:
            assert np.array_equal(_bits(off["tensors"][k]), _bits(on["tensors"][k])), (rank, k)
        for l in range(3):
            assert np.array_equal(_bits(off["W"][l]), _bits(on["W"][l])) and np.array_equal(_bits(off["dW"][l]), _bits(on["dW"][l])), (rank, l)
        assert on["seen"] == off["seen"] and len(on["seen"]) == 5 * epochs, (rank, len(on["seen"]))
        assert off["fused"][0] == 2 * epochs and off["fused"][2] == 3 * epochs and off["rw"] == (0, 0), (rank, off["fused"], off["rw"])
        assert on["fused"][0] == 5 * epochs and on["fused"][2] == 0 and on["rw"][0] == 3 * epochs and on["rw"][1] > 0, (rank, on["fused"], on["rw"])


# ---- 4. refused arguments, the single partition ------------------------------------------------------------------------------------------
def test_refused_arguments_and_single_partition(da):
    import aggregate_ref as ar
    from helpers import make_ctx
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="error -1.*halo_fused_pack_rowwise.*dory_configure first"):
        c.halo_fused_pack_rowwise(1)                   # before dory_configure
    c.configure(da.GCN, [4, 41, 2], 100, 0, 2)
    c.halo_fused_pack_rowwise(1)                       # any time after it
    c.halo_fused_pack_rowwise(0)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="error -1.*halo_fused_pack_rowwise"):
            c.halo_fused_pack_rowwise(bad)
    assert c.halo_fused_pack_rowwise_stats() == (0, 0)
    c.close()
    # a single partition: accepted and inert; refused while an epoch graph is being recorded
    one = make_ctx(da, ar.graph("uniform:64:300"), [16, 8, 2], 64, options={"gcn_transform_first": 2})
    one.halo_fused_pack(1)
    one.halo_fused_pack_rowwise(1)
    one.upload(0, "aTg", np.ones((64, 8), np.float32))
    one.upload(0, "z", np.ones((64, 8), np.float32))
    one.apply_vertex(0, da.BACKWARD)
    one.halo_exchange(0, da.BACKWARD)
    one.sync()
    assert one.halo_fused_pack_rowwise_stats() == (0, 0) and one.halo_fused_pack_stats() == (0, 0, 0)
    one.epoch_graph_begin()
    with pytest.raises(da.DoryError, match="error -1.*epoch graph is being recorded"):
        one.halo_fused_pack_rowwise(0)
    one.epoch_graph_drop()
    one.halo_fused_pack_rowwise(0)
    one.close()
