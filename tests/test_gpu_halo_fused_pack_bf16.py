"""dory_halo_fused_pack_bf16 (include/dorylus_hip.h): with dory_halo_fused_pack and dory_halo_bf16_rows both on, the K2 GEMM that
produces the rows of an exchange that ships bf16 (csrc/gemm.hip: gemm_dma_send16_kernel*, splitk_reduce_send16_kernel) rounds them
in its epilogue and writes them into the send buffer; the exchange runs no pack kernel.  Every comparison is bit for bit.

  1. stage level, on the rig of tests/test_gpu_halo_fused_pack.py (rank 0 of 4, a host transport that records what travels): the
     bytes are what dory_halo_pack -- gather_rows_bf16_kernel -- writes for the tensor as it is, and what tests/halo_bf16_ref.py
     packs from the downloaded tensor; counts and offsets in floats (rows x row_elems / 2); the product keeps the bits of the run
     with every switch off; the four counter sets; a second exchange and the switch off are counted fallbacks with the same bytes;
     the named rounding patterns through the epilogue; a one-column tensor packs;
  2. every way the stamp can go stale between producer and exchange: the current tensor in the current wire format travels, and
     the counters say which path ran;
  3. epochs over the in-process transport, the new switch off against on: GCN on the golden partitions (gather modes 1 and 2,
     exact rows, twins, three layers of odd widths, the transform-first order) and the GAT prototype -- the same bits everywhere,
     the counters what the rule predicts; the inert cases;
  4. the host transport (plain and direct plans, twins on) and the scatter transport in two processes;
  5. refused arguments, the single partition."""
import itertools
import os
import sys
import traceback

import numpy as np
import pytest

import halo_bf16_ref as hb
from test_gpu_halo_fused_pack import COLS, FORMS, MS, P, Rig, _bits, _free_port, _golden, _send_lists

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KS = (16, 130, 256, 602)      # 256 and 602 take the split-K path (pick_splits: K >= 256 with few tiles), 16 and 130 do not
GUARD = 64                    # bytes behind a reference buffer


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


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


def _gather_mode(rig, mode):
    if rig.form == "z":
        rig.ctx.gat_bf16_gather(mode)
    else:
        rig.ctx.set_option("gcn_bf16_gather", mode)


class Probe:
    """the rig's context seen through all four counter sets, and the reference bytes of dory_halo_pack (which follows the rule)"""

    def __init__(self, rig):
        import torch
        self.rig, self.ctx, self.torch = rig, rig.ctx, torch
        ld = max(4, rig.cols if rig.cols <= 1 else (rig.cols + 31) // 32 * 32)
        self.cap = (max(1, sum(len(l) for l in _send_lists(rig.M, 0))) + 8) * ld * 4      # fp32 rows of the longer plan and to spare

    def counters(self):
        c = self.ctx
        return {"fused": np.array(c.halo_fused_pack_stats(), np.int64), "f16": np.array(c.halo_fused_pack_bf16_stats(), np.int64),
                "bf16": np.array(c.halo_bf16_rows_stats(), np.int64),
                "packed": np.array([int(c.get_option("halo_rows_packed")), int(c.get_option("halo_floats_packed"))], np.int64)}

    def wire(self):
        eb, re = self.ctx.halo_wire_row(self.rig.xl, self.rig.xdir)
        return eb, re

    def kernel_pack(self):
        """dory_halo_pack of the exchange into a guarded device buffer: the bytes of the pack kernel the rule picks, as uint8"""
        eb, re = self.wire()
        n = self.rig.total * re * eb
        assert n + GUARD <= self.cap + GUARD
        buf = self.torch.full((self.cap + GUARD,), 0x5A, dtype=self.torch.uint8, device="cuda")
        self.torch.cuda.synchronize()
        assert buf.data_ptr() % 16 == 0
        self.ctx.halo_pack(self.rig.xl, self.rig.xdir, buf.data_ptr())
        self.ctx.sync()
        got = buf.cpu().numpy()
        assert (got[n:] == 0x5A).all(), "the reference pack wrote behind its rows"
        return got[:n].copy()

    def check(self, path, what):
        """one exchange: the current tensor's rows travel in the current wire format, laid out as the pack kernel would, counts and
        offsets in floats; `path` says which counters move: "fused16" / "fused32" (no pack kernel), "pack16" / "pack32" (a counted
        fallback), "off16" / "off32" (dory_halo_fused_pack off: a pack, nothing counted by the fused pack)"""
        rig, ctx = self.rig, self.ctx
        eb, re = self.wire()
        assert eb == (2 if path.endswith("16") else 4), (what, path, eb)
        want = self.kernel_pack()
        rows_on = int(self._rows_on)                                # (dory_halo_bf16_rows on: an fp32 exchange counts in fp32_packs_while_on)
        before = self.counters()
        send, sc, so = rig.exchange()
        fl = re * eb // 4                                           # floats a row: rows x row_elems / 2 for bf16
        assert sc == [len(l) * fl for l in rig.lists], (what, sc)
        assert so == [int(x) * fl for x in np.cumsum([0] + [len(l) for l in rig.lists[:-1]])], (what, so)
        got = np.ascontiguousarray(send, np.float32).view(np.uint8)
        assert got.size == want.size == rig.total * re * eb, (what, got.size, want.size)
        assert np.array_equal(got, want), (what, path, "bytes on the wire", int((got != want).sum()))
        if eb == 2:                                                 # ... and the numpy layout of the tensor as it is
            x = ctx.download(*rig.src)
            ref = hb.pack(x, np.concatenate([np.asarray(l, np.int64) for l in rig.lists]), rig.cols, bool(ctx.get_option("halo_exact_rows")))
            assert np.array_equal(got.view(np.uint16), ref), (what, path, "against halo_bf16_ref.pack")
        T, nbytes = rig.total, rig.total * re * eb
        d = {k: (v - before[k]).tolist() for k, v in self.counters().items()}
        kind = path[:-2]
        want_d = {
            "fused": [1, T, 0] if kind == "fused" else [0, 0, 1] if kind == "pack" else [0, 0, 0],
            "f16": [1, T] if path == "fused16" else [0, 0],
            "bf16": [1, nbytes, 0] if eb == 2 else [0, 0, rows_on],
            "packed": [0, 0] if kind == "fused" else [T, T * fl],
        }
        assert d == want_d, (what, path, d, want_d)

    _rows_on = True


def _all_on(rig, mode=2):
    _gather_mode(rig, mode)
    rig.ctx.halo_bf16_rows(1)
    rig.ctx.halo_fused_pack(1)
    rig.ctx.halo_fused_pack_bf16(1)


# ---- 1. stage level ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,cols,K,form", CASES, ids=[f"M{m}-c{c}-K{k}-{f}" for m, c, k, f in CASES])
def test_epilogue_writes_the_bf16_pack_kernels_bytes(da, M, cols, K, form):
    for variant in ((0, 1) if (M + cols + K) % 2 else (0,)):          # the plan with an empty peer: every other case
        rig = Rig(da, M, cols, K, form, variant)
        ctx, pr = rig.ctx, Probe(rig)
        assert ctx.halo_fused_pack_bf16_stats() == (0, 0)
        rig.produce()                                              # every switch off: the reference bits of the product
        ref = _bits(ctx.download(*rig.src))
        _all_on(rig)
        for exact in (0, 1):
            ctx.set_option("halo_exact_rows", exact)
            assert pr.wire() == (2, hb.row_elems(cols, bool(exact)))
            rig.produce()
            pr.check("fused16", (variant, exact, "fused"))          # (the reference pack in between left the stamp alone)
            assert np.array_equal(_bits(ctx.download(*rig.src)), ref), (variant, exact, "the product's bits")
            pr.check("pack16", (variant, exact, "second exchange of the same rows: the stamp was consumed"))
            ctx.halo_fused_pack_bf16(0)                            # the new switch off: as before it existed
            rig.produce()
            pr.check("pack16", (variant, exact, "new switch off: the bf16 pack kernel, a fallback of the fused pack"))
            assert np.array_equal(_bits(ctx.download(*rig.src)), ref), (variant, exact, "the product's bits, switch off")
            ctx.halo_fused_pack_bf16(1)
        ctx.close()


@pytest.mark.parametrize("M,cols", [(129, 41), (31, 130), (31, 256)], ids=["narrow", "wide", "splitk"])
def test_named_rounding_patterns_through_the_epilogue(da, M, cols):
    """z = h I: the finite bit patterns of halo_bf16_ref (ties, denormals, +-0, +-FLT_MAX among them) reach the epilogue's
    conversion; what travels is what the pack kernel makes of the tensor as produced"""
    rig = Rig(da, M, cols, cols, "z")
    ctx, pr = rig.ctx, Probe(rig)
    ctx.weight_set(0, "w", np.eye(cols, dtype=np.float32))
    ctx.upload(0, "h", hb.patterns(M * cols, seed=cols, finite=True).reshape(M, cols))
    _all_on(rig)
    for exact in (0, 1):
        ctx.set_option("halo_exact_rows", exact)
        rig.produce()
        z = ctx.download(0, "z")
        named = hb.named_patterns()
        named = named[((named >> 23) & 0xFF) != 0xFF]
        normal = named[((named >> 23) & 0xFF) != 0]                # (denormal inputs may be flushed by the matrix unit: not required)
        assert np.isin(normal[normal != 0x80000000], _bits(z)).all(), "the named patterns did not survive the identity product"
        pr.check("fused16", (cols, exact))
    ctx.close()


def test_one_column_tensor_is_a_counted_fallback(da):
    """ld == 1: a wire row of 4 elements is wider than the tensor's row, so no epilogue may write it.  (K2 itself takes no
    one-column operand -- its DMA moves 16-byte pieces -- so the rows of this tensor come from an upload.)"""
    rig = Rig(da, 31, 1, 16, "z")
    ctx, pr = rig.ctx, Probe(rig)
    _all_on(rig)
    for exact in (0, 1):
        ctx.set_option("halo_exact_rows", exact)
        assert pr.wire() == (2, 4)
        ctx.upload(0, "z", hb.patterns(31, seed=exact, finite=True).reshape(31, 1))
        pr.check("pack16", ("one column", exact))
    ctx.close()


# ---- 2. stale stamps --------------------------------------------------------------------------------------------------------------
def test_stale_stamps_fall_back_with_the_current_wire(da):
    rig = Rig(da, 129, 41, 16, "h", both_dirs=True)
    ctx, pr = rig.ctx, Probe(rig)
    _all_on(rig)
    rig.produce()
    pr.check("fused16", "nothing in between")
    # the gather mode changed: the wire is fp32 now, the stamp holds bf16 rows
    rig.produce()
    ctx.set_option("gcn_bf16_gather", 0)
    pr.check("pack32", "gcn_bf16_gather = 0 in between")
    rig.produce()                                                  # ... and the producer under mode 0 writes fp32 rows
    pr.check("fused32", "gather mode 0: an fp32 fused exchange")
    rig.produce()
    ctx.set_option("gcn_bf16_gather", 2)                           # fp32 rows in the buffer, a bf16 wire
    pr.check("pack16", "gcn_bf16_gather back to 2 in between")
    rig.produce()
    ctx.set_option("gcn_bf16_gather", 0)
    ctx.set_option("gcn_bf16_gather", 2)                           # there and back: the rows in the buffer are the wire's again
    pr.check("fused16", "gcn_bf16_gather 0 and back")
    # dory_halo_bf16_rows off / on
    rig.produce()
    ctx.halo_bf16_rows(0)
    pr._rows_on = False
    pr.check("pack32", "dory_halo_bf16_rows(0) in between")
    rig.produce()
    ctx.halo_bf16_rows(1)
    pr._rows_on = True
    pr.check("pack16", "dory_halo_bf16_rows(1) in between")
    # dory_halo_bf16_ghosts toggled
    for on in (1, 0):
        rig.produce()
        ctx.halo_bf16_ghosts(on)
        pr.check("pack16", ("dory_halo_bf16_ghosts in between", on))
    # the new switch itself, and dory_halo_fused_pack
    rig.produce()
    ctx.halo_fused_pack_bf16(0)
    pr.check("pack16", "dory_halo_fused_pack_bf16(0) in between")
    ctx.halo_fused_pack_bf16(1)
    pr.check("pack16", "on again, nothing produced since")
    rig.produce()
    ctx.halo_fused_pack(0)
    pr.check("off16", "dory_halo_fused_pack(0) in between")
    ctx.halo_fused_pack(1)
    # halo_exact_rows changed: 64 elements a row in the buffer, 44 on the wire
    rig.produce()
    ctx.set_option("halo_exact_rows", 1)
    pr.check("pack16", "halo_exact_rows changed in between")
    rig.produce()
    pr.check("fused16", "exact rows")
    # an upload of the source
    rig.produce()
    new = np.random.default_rng(1).uniform(-1, 1, (129, 41)).astype(np.float32)
    ctx.upload(0, "h", new)
    pr.check("pack16", "dory_tensor_upload in between")
    sent = np.ascontiguousarray(rig.sent[-1][0], np.float32).view(np.uint16).reshape(rig.total, 44)[:, :41]
    assert np.array_equal(sent, hb.round_bits(new[np.concatenate(rig.lists).astype(np.int64)]))
    # a pack of another exchange into the internal buffer
    rig.produce()
    before = pr.counters()["fused"]
    ctx.halo_exchange(1, da.BACKWARD)                              # grad@1: nobody produced it
    pr.check("pack16", "another exchange in between")
    assert (pr.counters()["fused"] - before).tolist() == [0, 0, 2]
    # a new plan (other lists: the slots move)
    rig.produce()
    rig.lists = _send_lists(129, 1)
    rig.total = sum(len(l) for l in rig.lists)
    rig.plan(da.FORWARD)
    pr.check("pack16", "dory_halo_plan in between")
    rig.produce()
    pr.check("fused16", "the new plan's map")
    # the raw pointer handed out: this tensor packs from now on
    rig.produce()
    assert ctx.info(0, "h")[3]
    pr.check("pack16", "raw pointer handed out after the producer")
    rig.produce()
    pr.check("pack16", "raw pointer: sticky")
    ctx.close()


# ---- 3. epochs over the in-process transport ------------------------------------------------------------------------------------------
def _same_bits(a, b, what):
    for r in range(len(a["tensors"])):
        assert set(a["tensors"][r]) == set(b["tensors"][r]), (what, r)
        for k in a["tensors"][r]:
            assert np.array_equal(_bits(a["tensors"][r][k]), _bits(b["tensors"][r][k])), (what, r, k)
        for l in range(len(a["weights"][r])):
            for nm in a["weights"][r][l]:
                assert np.array_equal(_bits(a["weights"][r][l][nm]), _bits(b["weights"][r][l][nm])), (what, r, l, nm, "W")
                assert np.array_equal(_bits(a["wgrads"][r][l][nm]), _bits(b["wgrads"][r][l][nm])), (what, r, l, nm, "dW")


def _run(da, gnn, case, dims, epochs, opts, on16, dl, mode=0, twins=0, heads=None, rows=1, seed=5):
    """one run_local of `epochs` epochs with dory_halo_fused_pack and dory_halo_bf16_rows (`rows`) on and the new switch as asked;
    returns (run_local's result, {rank: counters just before the context closes})"""
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
        if gnn == da.GAT and mode:
            ctx.gat_bf16_gather(mode)
        ctx.halo_fused_pack(1)
        ctx.halo_bf16_rows(rows)
        if twins:
            ctx.halo_bf16_ghosts(1)
        ctx.halo_fused_pack_bf16(on16)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {"fused": ctx.halo_fused_pack_stats(), "f16": ctx.halo_fused_pack_bf16_stats(), "bf16": ctx.halo_bf16_rows_stats(),
                           "rows": int(ctx.get_option("halo_rows_packed"))}
            close()
        ctx.close = closing
    if gnn == da.GCN:
        opts = dict(opts, gcn_bf16_gather=mode)
    out = run_local(da, pobjs, parts, dims, gnn, epochs, setup, opts, downloads=dl,
                    pre=(lambda c: c.gatmh_heads(heads)) if heads else None, wnames=("w", "a_l", "a_r") if heads else None)
    return out, kept


def _off_on(da, gnn, case, dims, epochs, opts, dl, what, **kw):
    off, koff = _run(da, gnn, case, dims, epochs, opts, 0, dl, **kw)
    on, kon = _run(da, gnn, case, dims, epochs, opts, 1, dl, **kw)
    _same_bits(off, on, what)
    assert set(koff) == set(kon)
    for r in koff:
        assert koff[r]["f16"] == (0, 0), (what, r, koff[r])
        assert koff[r]["bf16"] == kon[r]["bf16"], (what, r, "what travelled as bf16 is counted the same", koff[r], kon[r])
        assert sum(koff[r]["fused"][::2]) == sum(kon[r]["fused"][::2]), (what, r, "exchanges made", koff[r], kon[r])
    return on, koff, kon


def _gcn_dl(L, tf=False):
    dl = [(l, "z") for l in range(L)] + [(l, nm) for l in range(L - 1) for nm in ("h", "aTg")]
    if tf:
        return dl + [(l, "bgg") for l in range(L)] + [(l, nm) for l in range(1, L) for nm in ("xw", "fgxw")]
    return dl + [(l, "ah") for l in range(L)] + [(l, nm) for l in range(1, L) for nm in ("grad", "fg")] + [(l, "bg") for l in range(L - 1)]


def _check_gcn(on, koff, kon, epochs, L, mode, what):
    """aggregate-first: h@l forward (l < L - 1) and grad@l backward (l >= 1) are GEMM outputs -- L - 1 exchanges each way an epoch,
    the forward ones bf16 under mode >= 1, the backward ones under mode 2; whatever ships fp32 still fuses as fp32"""
    n16 = epochs * (L - 1) * (2 if mode == 2 else 1)
    for r, vw in enumerate(on["views"]):
        if not int(vw["localVtxCnt"]):
            continue
        assert kon[r]["fused"][0] == epochs * 2 * (L - 1) and kon[r]["fused"][2] == 0, (what, r, kon[r])
        assert kon[r]["f16"][0] == n16 and kon[r]["bf16"][0] == n16, (what, r, kon[r])
        assert koff[r]["fused"][0] == epochs * 2 * (L - 1) - n16 and koff[r]["fused"][2] == n16, (what, r, koff[r])
        assert kon[r]["rows"] == koff[r]["rows"] - kon[r]["f16"][1], (what, r, "rows through a pack kernel", kon[r], koff[r])


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty", "parts_toy60_p4_hash", "parts_toy97_p8_und"])
@pytest.mark.parametrize("mode", [1, 2])
def test_gcn_epochs_same_bits_and_every_bf16_exchange_fused(da, case, mode):
    dims, epochs = [20, 41, 6], 2
    for exact, twins in ((0, 0), (1, 1), (1, 0), (0, 1)) if case == "parts_toy60_p2" else ((mode - 1, 2 - mode),):
        what = (case, mode, exact, twins)
        opts = {"spmm_blk_nb": 8, "halo_exact_rows": exact}
        on, koff, kon = _off_on(da, da.GCN, case, dims, epochs, opts, _gcn_dl(2), what, mode=mode, twins=twins)
        _check_gcn(on, koff, kon, epochs, 2, mode, what)
        assert sum(k["f16"][1] for k in kon.values()) > 0, what


@pytest.mark.parametrize("mode", [1, 2])
def test_gcn_three_layers_odd_widths(da, mode):
    dims, epochs = [33, 25, 6, 3], 2
    for exact in (0, 1):
        what = ("odd widths", mode, exact)
        on, koff, kon = _off_on(da, da.GCN, "parts_toy60_p4_hash", dims, epochs, {"spmm_blk_nb": 8, "halo_exact_rows": exact}, _gcn_dl(3),
                                what, mode=mode, twins=exact)
        _check_gcn(on, koff, kon, epochs, 3, mode, what)


def _directed_parts(da, Pn=2, seed=17, V=240, E=2600):
    """partitions built from directed records: the golden ones carry symmetrised edge values, with which the library keeps the
    aggregate-first order whatever the option says"""
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % Pn).astype(np.int32)
    return lambda: ([da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, Pn) for r in range(Pn)], parts)


@pytest.mark.parametrize("mode", [1, 2])
def test_gcn_transform_first_xw_fused_as_bf16(da, mode):
    """every layer of 33-25-6-3 narrows: xw@1 and xw@2 (GEMM outputs) travel forward as bf16 rows an epilogue wrote; g (the tanh
    backward's output) travels backward through a pack kernel, bf16 under mode 2"""
    dims, epochs = [33, 25, 6, 3], 2
    for exact in (0, 1):
        what = ("transform first", mode, exact)
        opts = {"spmm_blk_nb": 8, "gcn_transform_first": 2, "halo_exact_rows": exact}
        on, koff, kon = _off_on(da, da.GCN, _directed_parts(da), dims, epochs, opts, _gcn_dl(3, tf=True), what, mode=mode, twins=1 - exact)
        for r in kon:
            assert kon[r]["f16"][0] == epochs * 2 and kon[r]["fused"][0] == epochs * 2 and kon[r]["fused"][2] >= epochs * 2, (what, r, kon[r])
            assert koff[r]["fused"][0] == 0, (what, r, koff[r])


@pytest.mark.parametrize("mode", [1, 2])
def test_gat_prototype_epochs(da, mode):
    """z@0, z@1 (forward) and grad@0 (dory_apply_vertex backward) are GEMM outputs, the last layer's grad comes from the softmax:
    three fused exchanges and one fallback an epoch; forward ships bf16 under mode >= 1, backward under mode 2"""
    dims, epochs, L = [20, 16, 6], 2, 2
    dl = [(l, nm) for l in range(L) for nm in ("z", "ah", "grad", "aTg", "fg_z", "bg_d")]
    for reuse in (1, 0):
        what = ("GAT prototype", mode, reuse)
        opts = {"spmm_blk_nb": 8, "gat_reuse_nsum": reuse, "halo_exact_rows": reuse}
        on, koff, kon = _off_on(da, da.GAT, "parts_toy60_p2", dims, epochs, opts, dl, what, mode=mode, twins=reuse, seed=11)
        n16 = epochs * (3 if mode == 2 else 2)
        for r in kon:
            assert kon[r]["fused"][0] == epochs * 3 and kon[r]["fused"][2] == epochs and kon[r]["f16"][0] == n16, (what, r, kon[r])
            assert koff[r]["fused"][0] == epochs * 3 - n16 and koff[r]["fused"][2] == epochs + n16, (what, r, koff[r])


def test_inert_cases_count_nothing(da):
    dims, epochs = [20, 41, 6], 2
    # gather mode 0: nothing ships bf16, every exchange fuses as fp32
    on, koff, kon = _off_on(da, da.GCN, "parts_toy60_p2", dims, epochs, {"spmm_blk_nb": 8}, _gcn_dl(2), "gather mode 0", mode=0)
    for r in kon:
        assert kon[r]["f16"] == (0, 0) and kon[r]["fused"] == koff[r]["fused"] and kon[r]["fused"][0] == 2 * epochs, ("gather mode 0", kon[r])
    # dory_halo_bf16_rows off under gather mode 2: likewise
    on, koff, kon = _off_on(da, da.GCN, "parts_toy60_p2", dims, epochs, {"spmm_blk_nb": 8}, _gcn_dl(2), "rows switch off", mode=2, rows=0)
    for r in kon:
        assert kon[r]["f16"] == (0, 0) and kon[r]["fused"] == koff[r]["fused"] and kon[r]["fused"][0] == 2 * epochs, ("rows switch off", kon[r])
    # a direct plan over the in-process transport (the peers read the send buffer on their own streams): never fused, twins or not
    for twins in (0, 1):
        what = ("direct plan, in-process", twins)
        on, koff, kon = _off_on(da, da.GCN, "parts_toy60_p2", dims, epochs, {"spmm_blk_nb": 8, "halo_direct_recv": 1}, _gcn_dl(2), what,
                                mode=2, twins=twins)
        for r in kon:
            assert kon[r]["f16"] == (0, 0) and kon[r]["fused"] == koff[r]["fused"] == (0, 0, 2 * epochs), (what, kon[r])
            assert kon[r]["bf16"][0] == (2 * epochs if twins else 0), (what, kon[r])
    # the multi-head GAT: its rule never ships bf16
    mh_dims, heads = [20, 128, 6], [8, 1]
    dl = [(l, nm) for l in range(2) for nm in ("z", "o", "dz", "fg_z", "bg_do", "bg_st")] + [(1, "logits")]
    on, koff, kon = _off_on(da, da.GATMH, "parts_toy60_p2", mh_dims, 1, {"spmm_blk_nb": 8}, dl, "8-head GAT", heads=heads, seed=11)
    for r in kon:
        assert kon[r]["f16"] == (0, 0) and kon[r]["bf16"][:2] == (0, 0) and kon[r]["fused"] == koff[r]["fused"] and kon[r]["fused"][0] == 2, kon[r]


# ---- 4. the host transport and the scatter transport, two processes ---------------------------------------------------------------------
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
        dims, epochs = [20, 41, 6], 2
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

        def run(transport, direct, on16):
            ctx = da.Context(0)
            ctx.configure(da.GCN, dims, V, rank, world)
            for k, v in (("spmm_blk_nb", 8), ("halo_direct_recv", direct), ("gcn_bf16_gather", 2)):
                ctx.set_option(k, v)
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
            ctx.halo_bf16_rows(1)
            ctx.halo_bf16_ghosts(1)
            ctx.halo_fused_pack_bf16(on16)
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
            eng.run(epochs)
            ctx.sync()
            res = {"seen": seen, "fused": ctx.halo_fused_pack_stats(), "f16": ctx.halo_fused_pack_bf16_stats(), "bf16": ctx.halo_bf16_rows_stats(),
                   "ghosts": ctx.halo_bf16_ghosts_stats(), "tensors": {}, "W": [], "dW": []}
            for l, nm in ((0, "ah"), (1, "ah"), (0, "h"), (0, "aTg"), (1, "grad"), (1, "fg"), (0, "bg")):
                if ctx.info(l, nm, ptr=False)[0]:
                    res["tensors"][(l, nm)] = ctx.download(l, nm)
            for l in range(L):
                res["W"].append(ctx.weight_get(l))
                res["dW"].append(ctx.weight_grad_get(l))
            eng.close()
            ctx.close()
            return res
        out = {(t, d, on): run(t, d, on) for t, d in (("host", 0), ("host", 1), ("scatter", 0)) for on in (0, 1)}
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, out))
    except Exception:
        q.put((rank, traceback.format_exc()))


def test_host_transport_two_processes_and_scatter_transport_inert():
    """two processes on one GPU, the bytes over gloo, twins on, two epochs under gather mode 2.  Host transport, plain and direct
    plans: every exchange ships bf16 rows an epilogue wrote (direct: they land in the peer's twin), the same counts, offsets and bits
    as with the new switch off.  Scatter transport: nothing fused, nothing counted."""
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
    res = [r for _, r in res]

    def same(a, b, what):
        assert set(a["tensors"]) == set(b["tensors"])
        for k in a["tensors"]:
            assert np.array_equal(_bits(a["tensors"][k]), _bits(b["tensors"][k])), (what, k)
        for l in range(2):
            assert np.array_equal(_bits(a["W"][l]), _bits(b["W"][l])) and np.array_equal(_bits(a["dW"][l]), _bits(b["dW"][l])), (what, l)
    for rank in (0, 1):
        for direct in (0, 1):
            off, on = res[rank][("host", direct, 0)], res[rank][("host", direct, 1)]
            what = ("host", rank, direct)
            same(off, on, what)
            assert on["seen"] == off["seen"] and len(on["seen"]) == 2 * epochs, what
            rows = sum(sum(c[0]) for c in on["seen"]) // 32          # 41 -> ld 64 bf16 = 32 floats a row
            assert rows > 0 and all(x % 32 == 0 for c in on["seen"] for x in c[0]), (what, on["seen"])
            assert on["fused"] == (2 * epochs, rows, 0) and on["f16"] == (2 * epochs, rows), (what, on["fused"], on["f16"])
            assert off["fused"] == (0, 0, 2 * epochs) and off["f16"] == (0, 0), (what, off["fused"], off["f16"])
            assert on["bf16"] == off["bf16"] == (2 * epochs, rows * 128, 0), (what, on["bf16"], off["bf16"])
            assert on["ghosts"] == off["ghosts"] and on["ghosts"]["landed_direct" if direct else "landed_by_kernel"] == 2 * epochs, (what, on["ghosts"])
        off, on = res[rank][("scatter", 0, 0)], res[rank][("scatter", 0, 1)]
        same(off, on, ("scatter", rank))
        assert on["seen"] == off["seen"] and sum(on["seen"]) > 0
        assert on["f16"] == (0, 0) and on["fused"] == off["fused"] == (0, 0, 2 * epochs) and on["bf16"] == off["bf16"] and on["bf16"][:2] == (0, 0)


# ---- 5. refused arguments, the single partition ------------------------------------------------------------------------------------------
def test_refused_arguments_and_single_partition(da):
    import aggregate_ref as ar
    from helpers import make_ctx
    c = da.Context(0)
    with pytest.raises(da.DoryError, match="error -1.*halo_fused_pack_bf16.*dory_configure first"):
        c.halo_fused_pack_bf16(1)                      # before dory_configure
    c.configure(da.GCN, [4, 41, 2], 100, 0, 2)
    c.halo_fused_pack_bf16(1)                          # any time after it
    c.halo_fused_pack_bf16(0)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="error -1.*halo_fused_pack_bf16"):
            c.halo_fused_pack_bf16(bad)
    with pytest.raises(da.DoryError):
        c.halo_fused_pack(2)                           # (stays refused)
    assert c.halo_fused_pack_bf16_stats() == (0, 0)
    c.close()
    # a single partition: accepted and inert; refused while an epoch graph is being recorded
    one = make_ctx(da, ar.graph("uniform:64:300"), [16, 41, 2], 64, options={"gcn_bf16_gather": 2})
    one.halo_fused_pack(1)
    one.halo_bf16_rows(1)
    one.halo_fused_pack_bf16(1)
    one.upload(0, "ah", np.ones((64, 16), np.float32))
    one.apply_vertex(0, da.FORWARD)
    one.halo_exchange(1, da.FORWARD)
    one.sync()
    assert one.halo_fused_pack_bf16_stats() == (0, 0) and one.halo_fused_pack_stats() == (0, 0, 0) and one.halo_bf16_rows_stats() == (0, 0, 0)
    one.epoch_graph_begin()
    with pytest.raises(da.DoryError, match="error -1.*epoch graph is being recorded"):
        one.halo_fused_pack_bf16(0)
    one.epoch_graph_drop()
    one.halo_fused_pack_bf16(0)
    one.close()
