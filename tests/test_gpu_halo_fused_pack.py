"""The fused halo pack (dory_halo_fused_pack, include/dorylus_hip.h): the K2 GEMM epilogues (csrc/gemm.hip: gemm_dma_send_kernel*,
splitk_reduce_send_kernel) write the send rows of the exchange that follows, which then skips its pack kernel.

Stage level: one context is rank 0 of P = 4 with a tiny hand-made adjacency and plan; a host transport's alltoallv callback records
the bytes that travel.  They must be byte for byte (padding included) what the existing pack kernel -- dory_halo_pack_tensor of the
same tensor into a device buffer -- writes, the counters must say that no pack kernel ran, and the produced tensor must have the
bits of the same call with the feature off.  Then every way the stamp can go stale: the bytes are always the current tensor's
rows, and the counters say which path ran.
Epochs: feature off against on over the in-process transport (GCN on the golden partitions, three layers of odd widths, the
transform-first order, the GAT prototype, the 8-head GAT, halo_direct_recv) and over the host transport in two processes:
identical bits everywhere, and the counters."""
import itertools
import os
import socket
import sys
import traceback

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = 4
MS = (1, 31, 128, 129, 300)
COLS = (7, 32, 41, 64, 65, 128, 130)
KS = (16, 130, 602)
FORMS = ("h", "z", "xw", "grad")


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _pad_ld(cols):
    return cols if cols <= 1 else (cols + 31) // 32 * 32


# ---- the cases: every (cols, form) pair and every (M, K) pair at least once -------------------------------------------------------
def _cases():
    out, seen_mk = [], set()
    for i, (cols, form) in enumerate(itertools.product(COLS, FORMS)):
        ks = [k for k in KS if form != "xw" or k > cols]        # xw = h W of a layer that narrows: its K is wider than its cols
        M, K = MS[i % len(MS)], ks[(i // len(MS) + i) % len(ks)]
        out.append((M, cols, K, form))
        seen_mk.add((M, K))
    for j, (M, K) in enumerate(sorted(set(itertools.product(MS, KS)) - seen_mk)):
        out.append((M, COLS[j % len(COLS)], K, "h" if j % 2 else "grad"))
    assert {(c, f) for _, c, _, f in out} == set(itertools.product(COLS, FORMS))
    assert {(m, k) for m, _, k, _ in out} == set(itertools.product(MS, KS))
    return out


CASES = _cases()


def _graph(M):
    """M local rows and three ghost rows on either side (one per peer); a few local edges, every ghost joined to row 0"""
    import aggregate_ref as ar
    rng = np.random.default_rng([7, M])
    E = min(4 * M, 400)
    s = np.concatenate([rng.integers(0, M, E), M + np.arange(3), np.zeros(3, np.int64)])
    d = np.concatenate([rng.integers(0, M, E), np.zeros(3, np.int64), M + np.arange(3)])
    w = rng.integers(1, 8, s.size).astype(np.float32) / 8
    return ar.graph_from_edges(M, 3, 3, s, d, w, np.ones(M, np.float32))


def _send_lists(M, variant):
    """variant 0: rows that go to 0, 1, 2 and 3 peers, unsorted, row 0 and row M - 1 listed, a row twice in one list;
    variant 1: the same with peer 2's list empty"""
    rng = np.random.default_rng([11, M, variant])
    if M == 1:
        lists = [[], [0], [0, 0], [0]]
    else:
        pool = rng.permutation(M)
        keep = pool[: max(2, (3 * M) // 4)]                       # the rest go nowhere
        lists = [[]]
        for q in range(1, P):
            n = max(1, len(keep) // (q + 1))
            l = rng.permutation(keep)[:n].tolist()
            lists.append(l)
        lists[1] += [0, M - 1, lists[1][0]]                       # row 0, row M - 1, and one row twice for one peer
        lists[2] += [M - 1, 0]
        lists[3] += [0, keep[0]]                                  # row 0 to all three peers
    if variant == 1:
        lists[2] = []
    return [[int(x) for x in l] for l in lists]


class Rig:
    """one context, rank 0 of 4, whose host transport records what every exchange sends"""

    def __init__(self, da, M, cols, K, form, variant=0, both_dirs=False):
        import torch
        from helpers import make_ctx
        self.da, self.M, self.cols, self.K, self.form, self.torch = da, M, cols, K, form, torch
        rng = np.random.default_rng([3, M, cols, K])
        gnn, opts = da.GCN, {}
        if form == "h":        # NN + tanh: h@0 = tanh(ah@0 W0), sent forward into fg@1
            dims, self.src, self.xl, self.xdir, self.prod = [K, cols, 2], (0, "h"), 1, da.FORWARD, (0, da.FORWARD)
            self.inp, self.wl = (0, "ah", K), 0
        elif form == "z":      # NN plain, the GAT prototype's z@0 = h@0 W0, sent forward into fg_z@0
            gnn = da.GAT
            dims, self.src, self.xl, self.xdir, self.prod = [K, cols, 2], (0, "z"), 1, da.FORWARD, (0, da.FORWARD)
            self.inp, self.wl = (0, "h", K), 0
        elif form == "xw":     # NN plain, transform-first: xw@1 = h@0 W1 (K = dims[1] > cols), sent forward into fgxw@1
            opts = {"gcn_transform_first": 2}
            dims, self.src, self.xl, self.xdir, self.prod = [4, K, cols], (1, "xw"), 1, da.FORWARD, (0, da.FORWARD)
            self.inp, self.wl = (0, "ah", 4), 1
        else:                  # NT: grad@1 = g@1 W1^T (K = the class count), sent backward into bg@0
            dims, self.src, self.xl, self.xdir, self.prod = [4, cols, K], (1, "grad"), 1, da.BACKWARD, (1, da.FORWARD)
            self.inp, self.wl = (1, "ah", cols), 1
        self.dims = dims
        ctx = self.ctx = make_ctx(da, _graph(M), dims, 4 * M + 8, gnn=gnn, node_id=0, num_nodes=P, options=opts)
        if form == "xw":
            assert ctx.transform_first_layer(1) and not ctx.transform_first_layer(0)
        self.lists = _send_lists(M, variant)
        self.total = sum(len(l) for l in self.lists)
        self.plan(self.xdir)
        if both_dirs:
            self.plan(1 - self.xdir)
        for l in range(2):
            ctx.weight_set(l, "w", (rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32))
        self.new_input(0)
        self.sent = []

        def alltoallv(send, sc, so, recv, rc, ro):
            n = int((so + sc).max())
            self.sent.append((np.array(send[:n], copy=True), [int(x) for x in sc], [int(x) for x in so]))
        ctx.set_host_transport(alltoallv, lambda buf: None)
        self.buf = torch.empty(max(self.total, 1) * _pad_ld(cols) + 64, dtype=torch.float32, device="cuda")

    def plan(self, direction):
        self.ctx.halo_plan(direction, self.lists, [[], [2], [0], [1]])

    def new_input(self, salt):
        layer, name, width = self.inp
        rng = np.random.default_rng([5, self.M, width, salt])
        self.ctx.upload(layer, name, rng.uniform(-1, 1, (self.M, width)).astype(np.float32))

    def produce(self):
        self.ctx.apply_vertex(*self.prod)

    def kernel_pack(self, w):
        """what the existing pack kernel makes of the source tensor as it is now: the reference for the bytes"""
        self.buf.fill_(-7.0)
        self.torch.cuda.synchronize()
        self.ctx.halo_pack_tensor(self.src[0], self.src[1], self.xdir, self.buf.data_ptr())
        self.ctx.sync()
        got = self.buf.cpu().numpy()
        assert (got[self.total * w:] == -7.0).all()
        return got[: self.total * w].copy()

    def exchange(self):
        n = len(self.sent)
        self.ctx.halo_exchange(self.xl, self.xdir)
        self.ctx.sync()
        assert len(self.sent) == n + 1
        return self.sent[-1]

    def stats(self):
        return np.array(self.ctx.halo_fused_pack_stats(), np.int64)

    def width(self):
        return self.cols if self.ctx.get_option("halo_exact_rows") else _pad_ld(self.cols)

    def check_exchange(self, want_delta, what):
        """the exchange sends the current tensor's rows as the pack kernel lays them out; the counters move by want_delta"""
        w = self.width()
        want = self.kernel_pack(w)
        before = self.stats()
        send, sc, so = self.exchange()
        assert sc == [len(l) * w for l in self.lists] and so == [int(x) * w for x in np.cumsum([0] + [len(l) for l in self.lists[:-1]])], what
        assert send.size == self.total * w, (what, send.size, self.total, w)
        assert np.array_equal(_bits(send), _bits(want)), (what, "bytes on the wire", int((_bits(send) != _bits(want)).sum()))
        assert (self.stats() - before).tolist() == list(want_delta), (what, before, self.stats())


@pytest.mark.parametrize("M,cols,K,form", CASES, ids=[f"M{m}-c{c}-K{k}-{f}" for m, c, k, f in CASES])
def test_epilogue_writes_the_pack_kernels_bytes(da, M, cols, K, form):
    for variant in ((0, 1) if (M + cols + K) % 2 else (0,)):          # the plan with an empty peer: every other case
        rig = Rig(da, M, cols, K, form, variant)
        ctx = rig.ctx
        assert rig.stats().tolist() == [0, 0, 0]
        rig.produce()                                              # the feature off: the reference bits of the product
        ref = _bits(ctx.download(*rig.src))
        rig.check_exchange((0, 0, 0), (variant, "off"))           # ... and nothing is counted while it is off
        for exact in (0, 1):
            ctx.set_option("halo_exact_rows", exact)
            ctx.halo_fused_pack(1)
            rig.produce()
            rig.check_exchange((1, rig.total, 0), (variant, exact, "fused"))     # (the kernel pack in between left the stamp alone)
            assert np.array_equal(_bits(ctx.download(*rig.src)), ref), (variant, exact, "the product's bits")
            rig.check_exchange((0, 0, 1), (variant, exact, "second exchange of the same rows: the stamp was consumed"))
            ctx.halo_fused_pack(0)
        ctx.close()


def test_single_partition_and_bad_arguments(da):
    import aggregate_ref as ar
    from helpers import make_ctx
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="dory_configure first"):
        c.halo_fused_pack(1)
    c.close()
    one = make_ctx(da, ar.graph("uniform:64:300"), [16, 41, 2], 64)
    with pytest.raises(da.DoryError):
        one.halo_fused_pack(2)
    one.halo_fused_pack(1)
    one.upload(0, "ah", np.ones((64, 16), np.float32))
    one.apply_vertex(0, da.FORWARD)
    one.halo_exchange(1, da.FORWARD)
    one.sync()
    assert one.halo_fused_pack_stats() == (0, 0, 0)
    one.close()


def test_stale_stamps_fall_back(da):
    rig = Rig(da, 129, 41, 16, "h", both_dirs=True)
    ctx, T = rig.ctx, rig.total
    ctx.halo_fused_pack(1)
    rng = np.random.default_rng(1)
    # (d) a kernel pack into a caller's buffer in between (check_exchange makes one): still fused
    rig.produce()
    rig.check_exchange((1, T, 0), "d: dory_halo_pack_tensor in between")
    # (f) the producer twice: the second call's rows, fused
    rig.produce()
    rig.new_input(1)
    rig.produce()
    rig.check_exchange((1, T, 0), "f: produced twice")
    # (a) an upload of the source between producer and exchange: the new rows travel, packed by the kernel
    rig.produce()
    new = rng.uniform(-1, 1, (129, 41)).astype(np.float32)
    ctx.upload(0, "h", new)
    rig.check_exchange((0, 0, 1), "a: dory_tensor_upload")
    assert np.array_equal(_bits(rig.sent[-1][0].reshape(T, -1)[:, :41]), _bits(new[np.concatenate(rig.lists).astype(np.int64)]))
    # (b) dory_tensor_fill_uniform likewise
    rig.produce()
    ctx.fill_uniform(0, "h", 99)
    rig.check_exchange((0, 0, 1), "b: dory_tensor_fill_uniform")
    # an upload of ANOTHER tensor leaves the stamp alone
    rig.produce()
    ctx.upload(1, "ah", np.zeros((129, 41), np.float32))
    rig.check_exchange((1, T, 0), "an upload of another tensor")
    # (e) another exchange packs into the internal buffer in between
    rig.produce()
    before = rig.stats()
    ctx.halo_exchange(1, da.BACKWARD)          # grad@1: nobody produced it
    rig.check_exchange((0, 0, 1), "e: another exchange in between")
    assert (rig.stats() - before).tolist() == [0, 0, 2]
    # (g) switched off in between: the exchange packs, and nothing is counted while off; back on without a producer: a fallback
    rig.produce()
    ctx.halo_fused_pack(0)
    rig.check_exchange((0, 0, 0), "g: dory_halo_fused_pack(0)")
    ctx.halo_fused_pack(1)
    rig.check_exchange((0, 0, 1), "g: on again, nothing produced since")
    # (h) a new plan in between (other lists: the slots move)
    rig.produce()
    rig.lists = _send_lists(129, 1)
    rig.total = T = sum(len(l) for l in rig.lists)
    rig.plan(da.FORWARD)
    rig.check_exchange((0, 0, 1), "h: dory_halo_plan")
    rig.produce()
    rig.check_exchange((1, T, 0), "h: the new plan's map")
    # the width changes between producer and exchange: the stamp names the other width
    rig.produce()
    ctx.set_option("halo_exact_rows", 1)
    rig.check_exchange((0, 0, 1), "halo_exact_rows changed in between")
    rig.produce()
    rig.check_exchange((1, T, 0), "exact rows")
    # (c) the raw pointer handed out: this tensor packs from now on, whatever is produced
    rig.produce()
    assert ctx.info(0, "h")[3]
    rig.check_exchange((0, 0, 1), "c: raw pointer handed out after the producer")
    rig.produce()
    rig.check_exchange((0, 0, 1), "c: sticky")
    assert ctx.info(0, "h", ptr=False)[3] is None
    ctx.close()


def test_setting_the_transport_again_drops_the_stamp(da):
    rig = Rig(da, 31, 41, 16, "h")
    ctx = rig.ctx
    ctx.halo_fused_pack(1)
    rig.produce()
    tx = ctx._tx
    ctx.lib.dory_comm_set_host_transport(ctx.h, tx[0], tx[1], None)        # the transport set again: the stamp goes
    rig.check_exchange((0, 0, 1), "dory_comm_set_host_transport in between")
    rig.produce()
    rig.check_exchange((1, rig.total, 0), "fused again")
    ctx.close()


# ---- epochs ---------------------------------------------------------------------------------------------------------------------
def _golden(da, name):
    import glob
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


def _with_feature(setup, on, kept):
    """run_local's setup hook: the feature switched as asked (the plans exist by then); run_local closes its contexts, so the
    counters of every rank are read just before that"""
    def wrapped(ctx, r, g):
        setup(ctx, r, g)
        ctx.halo_fused_pack(on)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = ctx.halo_fused_pack_stats() + (int(ctx.get_option("halo_direct_recvs")) + int(ctx.get_option("halo_staged_recvs")),)
            close()
        ctx.close = closing
    return wrapped


def _same_bits(a, b, what):
    for r in range(len(a["tensors"])):
        assert set(a["tensors"][r]) == set(b["tensors"][r]), (what, r)
        for k in a["tensors"][r]:
            assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(len(a["weights"][r])):
            for nm in a["weights"][r][l]:
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


def _gcn_run(da, pobjs, parts, dims, epochs, opts, on, seed=5):
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
    tf = bool(opts.get("gcn_transform_first"))
    dl = [(l, "z") for l in range(L)] + [(l, nm) for l in range(L - 1) for nm in ("h", "aTg")]
    if not tf:
        dl += [(l, "ah") for l in range(L)] + [(l, nm) for l in range(1, L) for nm in ("grad", "fg")] + [(l, "bg") for l in range(L - 1)]
    kept = {}
    out = run_local(da, pobjs, parts, dims, da.GCN, epochs, _with_feature(setup, on, kept), opts, downloads=dl)
    return out, kept


def _gcn_off_on(da, make, dims, epochs, base, what, check):
    """feature off (overlap 1) against on with overlap 1 and 0: the same bits in every downloaded tensor, weight and gradient"""
    for exact in (0, 1):
        opts = dict(base, halo_exact_rows=exact)
        off, k_off = _gcn_run(da, *make(), dims, epochs, dict(opts, halo_overlap=1), 0)
        assert all(v[:3] == (0, 0, 0) for v in k_off.values()), (what, k_off)
        for overlap in (1, 0):
            on, k_on = _gcn_run(da, *make(), dims, epochs, dict(opts, halo_overlap=overlap), 1)
            _same_bits(off, on, (what, exact, overlap, "fused pack off / on"))
            for r, vw in enumerate(on["views"]):
                fused, rows, fallback, made = k_on[r]
                assert fused + fallback == made == k_off[r][3], (what, r, k_on[r], k_off[r])
                check(r, int(vw["localVtxCnt"]), fused, rows, fallback, made)


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty", "parts_toy60_p4_hash", "parts_toy97_p8_und"])
def test_gcn_epochs_same_bits_and_every_exchange_fused(da, case):
    dims, epochs = [20, 41, 6], 3
    L = len(dims) - 1

    def check(r, N, fused, rows, fallback, made):
        if N:
            assert fallback == 0 and fused == epochs * 2 * (L - 1), (case, r, fused, fallback)
    _gcn_off_on(da, lambda: _golden(da, case), dims, epochs, {"spmm_blk_nb": 8}, case, check)


def test_gcn_three_layers_odd_widths(da):
    dims, epochs = [33, 25, 6, 3], 3

    def check(r, N, fused, rows, fallback, made):
        if N:
            assert fallback == 0 and fused == epochs * 2 * 2, (r, fused, fallback)
    _gcn_off_on(da, lambda: _golden(da, "parts_toy60_p4_hash"), dims, epochs, {"spmm_blk_nb": 8}, "odd widths", check)


def _random_parts(da, Pn, seed=17, V=240, E=2600):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % Pn).astype(np.int32)
    return lambda: ([da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, Pn) for r in range(Pn)], parts)


def test_gcn_transform_first_xw_fused_g_falls_back(da):
    """every layer of 33-25-6-3 narrows: xw@1 and xw@2 (GEMM outputs) travel forward fused, g (the tanh backward's output) travels
    backward through the pack kernel"""
    dims, epochs = [33, 25, 6, 3], 2

    def check(r, N, fused, rows, fallback, made):
        assert N and fused == epochs * 2 and fallback == made - fused and fallback >= epochs * 2, (r, fused, fallback, made)
    _gcn_off_on(da, _random_parts(da, 2), dims, epochs, {"spmm_blk_nb": 8, "gcn_transform_first": 2}, "transform first", check)


def test_gcn_direct_recv_over_the_local_transport_falls_back(da):
    dims, epochs = [20, 41, 6], 2

    def check(r, N, fused, rows, fallback, made):
        assert fused == 0 and rows == 0 and fallback == made == epochs * 2, (r, fused, fallback, made)
    _gcn_off_on(da, lambda: _golden(da, "parts_toy60_p2"), dims, epochs, {"spmm_blk_nb": 8, "halo_direct_recv": 1}, "direct recv", check)


def test_gat_prototype_epoch(da):
    from local_ranks import run_local
    case, dims, L = "parts_toy60_p2", [20, 16, 6], 2
    runs = {}
    for on, overlap in ((0, 1), (1, 1), (1, 0)):
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
        kept = {}
        runs[(on, overlap)] = (run_local(da, pobjs, parts, dims, da.GAT, 1, _with_feature(setup, on, kept),
                                         {"spmm_blk_nb": 8, "halo_overlap": overlap}, downloads=dl), kept)
    for key in ((1, 1), (1, 0)):
        _same_bits(runs[(0, 1)][0], runs[key][0], ("GAT prototype", key))
        for r, (fused, rows, fallback, made) in runs[key][1].items():
            # z@0, z@1 forward and grad@0 (apply_vertex backward) are GEMM outputs; the last layer's grad comes from the softmax
            assert fused >= 1 and fused + fallback == made == runs[(0, 1)][1][r][3], (key, r, fused, fallback, made)
            assert fused == 3 and fallback == 1, (key, r, fused, fallback)


def test_gat_mh_epoch(da):
    from local_ranks import run_local
    Pn, dims, heads, V = 2, [40, 128, 41], [8, 1], 240
    make = _random_parts(da, Pn)
    rng = np.random.default_rng(18)
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
    runs = []
    for on in (0, 1):
        pobjs, parts = make()
        kept = {}
        runs.append((run_local(da, pobjs, parts, dims, da.GATMH, 1, _with_feature(setup, on, kept), {"spmm_blk_nb": 8}, downloads=dl,
                               pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r")), kept))
    _same_bits(runs[0][0], runs[1][0], "8-head GAT, fused pack off / on")
    for r, (fused, rows, fallback, made) in runs[1][1].items():
        # z@0 and z@1 forward fused; do / st of both layers' backward sweeps through the pack kernel
        assert fused >= 1 and fused + fallback == made == runs[0][1][r][3], (r, fused, fallback, made)
        assert fused == 2, (r, fused, fallback)


# ---- the host transport: two processes on one GPU (worker pattern of tests/test_gpu_halo_exact_rows.py) ----------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, on, direct, q):
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
        ctx = da.Context(0)
        ctx.configure(da.GCN, dims, V, rank, world)
        ctx.set_option("spmm_blk_nb", 8)
        ctx.set_option("halo_direct_recv", direct)
        if on:
            ctx.halo_fused_pack(1)             # before the plans: dory_halo_plan builds the maps
        part.upload(ctx, parts)
        ctx.preallocate()
        ctx.upload(0, "x", X[g["localToGlobal"]])
        if g["srcGhostCnt"]:
            ctx.upload(0, "fg", X[g["srcGhost"]].reshape(g["srcGhostCnt"], dims[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
        ctx.adam_config(0.01)

        def alltoallv(send, sc, so, recv, rc, ro):
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

        def allreduce(buf):
            t = torch.from_numpy(buf.copy())
            dist.all_reduce(t)
            buf[:] = t.numpy()
        ctx.set_host_transport(alltoallv, allreduce)
        eng = da.NativeEngine(ctx)
        eng.run(2)
        ctx.sync()
        res = {"stats": ctx.halo_fused_pack_stats(), "tensors": {}, "W": [], "dW": []}
        for l, nm in ((0, "ah"), (1, "ah"), (0, "h"), (0, "aTg"), (1, "grad"), (1, "fg"), (0, "bg")):
            if ctx.info(l, nm, ptr=False)[0]:
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


def _host_transport_run(on, direct):
    import torch.multiprocessing as mp
    world = 2
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = _free_port()
    procs = [ctxm.Process(target=_worker, args=(r, world, port, on, direct, q)) for r in range(world)]
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


@pytest.mark.parametrize("direct", [0, 1])
def test_host_transport_two_processes_fused_same_bits(direct):
    """two epochs, the bytes over gloo; halo_direct_recv changes the receive side only: every exchange is fused either way"""
    off, on = _host_transport_run(0, direct), _host_transport_run(1, direct)
    for rank in (0, 1):
        assert off[rank]["stats"] == (0, 0, 0)
        fused, rows, fallback = on[rank]["stats"]
        assert fused == 2 * 2 and fallback == 0 and rows > 0, (rank, on[rank]["stats"])
        assert set(off[rank]["tensors"]) == set(on[rank]["tensors"])
        for k in off[rank]["tensors"]:
            assert np.array_equal(_bits(off[rank]["tensors"][k]), _bits(on[rank]["tensors"][k])), (rank, k)
        for l in range(2):
            assert np.array_equal(_bits(off[rank]["W"][l]), _bits(on[rank]["W"][l])), (rank, l)
            assert np.array_equal(_bits(off[rank]["dW"][l]), _bits(on[rank]["dW"][l])), (rank, l)
