"""dory_gatmh_bf16_ghosts (include/dorylus_hip.h): on top of dory_halo_bf16_ghosts the multi-head GAT's fg_z and bg_do get bf16 twins;
rows that travel as bf16 (dory_halo_bf16_rows + dory_gatmh_halo_bf16 + option gatmh_bf16_gather) stay bf16 where the bf16 edge passes
gather them, dory_apply_edge forms fg_el / fg_er from the twin (csrc/gat_mh.hip: gatmh_scores4_bf16_kernel / gatmh_scores_bf16_kernel)
and the merged unpack keeps its do part bf16 (csrc/elementwise.hip: scatter_rows_pair_bf16_keep_kernel).

THE CONTRACT: two runs with dory_halo_bf16_rows, dory_gatmh_halo_bf16 and dory_halo_bf16_ghosts on, one with dory_gatmh_bf16_ghosts on too:
every local tensor, weight and gradient has the same bits, a download of fg_z / bg_do gives the same (rounded) rows.  Every comparison
below is bit for bit.  (Under a plan made with halo_direct_recv = 1 the switch also turns the wire from fp32 to bf16, as
dory_halo_bf16_ghosts does for the other models: the local results are compared there, on shapes whose kernels read no fg_el.)

  1. the scores kernels through dory_halo_unpack + dory_apply_edge;   2. the keep form of the merged unpack through dory_gatmh_bwd_pack / _unpack;
  3. stage by stage, the row-gather family, P = 2;   4. whole epochs over the in-process transport;   5. the sweep forms;
  6. readers of fp32 rows;   7. inert cases;   8. refusals;   9. the epoch graph."""
import threading

import numpy as np
import pytest

import gatmh_bf16_ghost_ref as gg
import gatmh_halo_bf16_ref as gr
import halo_bf16_ghost_ref as hg
import halo_bf16_ref as hb
import halo_exact_ref as hx
from test_gpu_gatmh_bf16_gather import backward_takes_the_sweep_forms, make_gatmh, make_params, same_bits
from test_gpu_gatmh_bwd_merged import _raw
from test_gpu_gatmh_row_gather import _dst_rowwise_covers, _hub_graph, _layer_shapes
from test_gpu_halo_bf16_ghosts import _poison_twin, _stats, _twin
from test_gpu_halo_bf16_rows import _own_views
from test_gpu_halo_exact_rows import _bits, _golden, _plan

pytestmark = pytest.mark.gpu
KEYS = ("fwd_kept", "bwd_kept", "bwd_kept_merged", "twin_reads_rows", "twin_reads_sweep", "scores_from_twin", "widened")
ZERO = dict.fromkeys(KEYS, 0)
GHOST_ZERO = dict(landed_direct=0, landed_by_kernel=0, conversions_skipped=0, widened=0)


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def _switches(ctx, gh, halo16=1):
    """the three switches of the contract, then the one under test"""
    ctx.halo_bf16_rows(1)
    ctx.gatmh_halo_bf16(halo16)
    ctx.halo_bf16_ghosts(1)
    ctx.gatmh_bf16_ghosts(gh)


def _rank0_of_2(da, dims, heads, G, seed, opts=None):
    """rank 0 of 2 on a partition of 64 local rows with G ghost rows on either side, inputs and weights from `seed`"""
    import aggregate_ref as ar
    g = ar.graph(hx.graph_name(G))
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (hx.N_LOCAL, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], hx.N_LOCAL).astype(np.uint32)
    return make_gatmh(da, g, dims, heads, int(g["globalVtxCnt"]) + 1, X, labels, make_params(rng, dims, heads), opts, 0, 2)


# ---- 1. the scores kernels -----------------------------------------------------------------------------------------------------------
# K x D: 8 x 16, 4 x 8 and 1 x 6 take the four-element form (a head on 4 / 2 lanes, one head on the whole row of 8 chunks), 3 x 32 (ld 96:
# 24 chunks, no power of two), 32 x 2 and 32 x 1 the scalar form -- the selection of launch_gatmh_scores
@pytest.mark.parametrize("G", [1, 63, 257])
@pytest.mark.parametrize("K,D", [(8, 16), (4, 8), (3, 32), (1, 6), (32, 2), (32, 1)])
def test_scores_from_twin_rows_equal_scores_from_widened_rows(da, K, D, G):
    import torch
    cols, dims, heads = K * D, [12, K * D, 3], [K, 1]
    ld = hx.pad_ld(cols)
    rng = np.random.default_rng([K, D, G])
    z = rng.uniform(-1, 1, (hx.N_LOCAL, cols)).astype(np.float32)
    wire = np.zeros((G, ld), np.uint16)                       # the padded wire row: ld elements, zeros behind cols
    wire[:, :cols] = hb.round_bits(rng.uniform(-2, 2, (G, cols)).astype(np.float32))
    wire[0, :min(cols, 4)] = hb.round_bits(np.array([1.0 + 2.0 ** -7, -0.0, 2.0 ** -130, -3.0e30], np.float32))[:min(cols, 4)]
    out = []
    for gh in (1, 0):
        ctx = _rank0_of_2(da, dims, heads, G, 5, {"gatmh_bf16_gather": 1})
        _switches(ctx, gh)
        _, slots = _plan(da, ctx, da.FORWARD, 3, G, cols)
        ctx.upload(0, "z", z)
        if gh:
            assert ctx.halo_wire_row(1, da.FORWARD) == (2, ld)
            buf = torch.from_numpy(wire.view(np.int16).copy()).cuda()
            torch.cuda.synchronize()
            _poison_twin(ctx, 0, "fg_z")
            ctx.halo_unpack(1, da.FORWARD, buf.data_ptr())
            got, state = _twin(ctx, 0, "fg_z")
            assert state == hg.TWIN and np.array_equal(got, hg.keep(np.zeros((G, ld), np.uint16), slots, wire, cols, False))
        else:                                                   # the widened rows as fp32 rows
            rows = np.zeros((G, cols), np.float32)
            rows[slots] = hb.widen(wire[:, :cols])
            ctx.upload(0, "fg_z", rows)
        ctx.apply_edge(1, da.FORWARD)
        s = ctx.gatmh_bf16_ghosts_stats()
        assert s == dict(ZERO, fwd_kept=gh, scores_from_twin=gh), (K, D, G, gh, s)
        assert ctx.halo_bf16_ghost_peek(0, "fg_z")[1] == (hg.TWIN if gh else hg.FP32)      # (nothing was widened for the scores)
        out.append({nm: ctx.download(0, nm) for nm in ("fg_el", "fg_er", "el", "er")})
        if gh:                                                  # a download shows the widened rows, and then both copies are current
            rows = np.zeros((G, cols), np.float32)
            rows[slots] = hb.widen(wire[:, :cols])
            assert same_bits(ctx.download(0, "fg_z"), rows)
            assert ctx.halo_bf16_ghost_peek(0, "fg_z")[1] == hg.BOTH and ctx.gatmh_bf16_ghosts_stats()["widened"] == 1
        ctx.close()
    assert out[0]["fg_el"].shape == (G, K) and np.isfinite(out[1]["fg_el"]).all()
    for nm in out[0]:
        assert same_bits(out[0][nm], out[1][nm]), (K, D, G, nm)


# ---- 2. the keep form of the merged unpack ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("G", [3, 257])
@pytest.mark.parametrize("hidden,last", [((8, 16), (1, 41)), ((4, 16), (2, 8)), ((32, 2), (1, 41))])
def test_merged_unpack_keeps_the_do_part_in_the_twin(da, hidden, last, G):
    """dory_gatmh_bwd_pack, then dory_gatmh_bwd_unpack of the very rows (as many sent as received), padded and exact: 8 x 16, 4 x 16,
    2 x 8, 32 x 2 and 1 x 41 (exact: w = 48 in an ld of 64)"""
    import torch
    from helpers import _poison_padding
    (K0, D0), (K1, C1) = hidden, last
    heads, dims, zw = [K0, K1], [12, K0 * D0, C1], [K0 * D0, K1 * C1]
    ctx = _rank0_of_2(da, dims, heads, G, 7, {"gatmh_bf16_gather": 2})
    _switches(ctx, 1)
    send, slots = _plan(da, ctx, da.BACKWARD, G, G, zw[0])
    rng = np.random.default_rng([K0, D0, G])
    expect = dict(ZERO)
    for exact in (0, 1):
        ctx.set_option("halo_exact_rows", exact)
        for l in range(2):
            K, cols = heads[l], zw[l]
            ld, ld_st = gr.pad_ld(cols), gr.pad_ld(4 * K)
            R, dof, k4, w = gr.wire_row(cols, K, exact)
            assert ctx.gatmh_bwd_wire_row(l) == (R, dof, k4) and ctx.gatmh_bwd_wire_do(l) == (2, w), (exact, l)
            do = hb.local_values(hx.N_LOCAL, cols, salt=l + 2 * exact)
            st = rng.uniform(0.5, 1.5, (hx.N_LOCAL, 4 * K)).astype(np.float32)
            ctx.upload(l, "do", do)
            ctx.upload(l, "st", st)
            buf = torch.zeros(max(G * R, 4), device="cuda")
            torch.cuda.synchronize()
            ctx.gatmh_bwd_pack(l, buf.data_ptr())
            ctx.sync()
            rows = buf.cpu().numpy()[:G * R]
            assert np.array_equal(_bits(rows), _bits(gr.pack(do, st, K, w, [send])))
            _poison_twin(ctx, l, "bg_do")
            _poison_padding(ctx, l, "bg_st")
            before = _stats(ctx)
            ctx.gatmh_bwd_unpack(l, buf.data_ptr())
            twin, state = _twin(ctx, l, "bg_do")
            want_twin, want_st = gg.unpack_keep(rows, K, w, [[], slots], G, ld, ld_st)
            assert state == hg.TWIN and np.array_equal(twin, want_twin), (exact, l, "twin")
            assert (twin[:, w:] == 0).all() and w <= ld
            assert np.array_equal(_bits(_raw(ctx, l, "bg_st")), _bits(want_st)), (exact, l, "bg_st")
            expect["bwd_kept_merged"] += 1
            assert ctx.gatmh_bf16_ghosts_stats() == expect and _stats(ctx) == dict(before, landed_by_kernel=before["landed_by_kernel"] + 1)
            dl = ctx.download(l, "bg_do")
            assert same_bits(dl, hb.widen(want_twin)[:, :cols]) and ctx.halo_bf16_ghost_peek(l, "bg_do")[1] == hg.BOTH
            expect["widened"] += 1
            assert ctx.gatmh_bf16_ghosts_stats() == expect
    # the same buffer (the last layer's, exact) with this switch off: the widening unpack leaves the rows the download above showed
    ctx.gatmh_bf16_ghosts(0)
    assert ctx.halo_bf16_ghost_peek(1, "bg_do") == (None, hg.FP32)
    ctx.halo_bf16_ghosts(1)
    ctx.gatmh_bwd_unpack(1, buf.data_ptr())
    assert same_bits(ctx.download(1, "bg_do"), dl) and ctx.gatmh_bf16_ghosts_stats() == expect
    ctx.close()


# ---- 3 / 6. stage by stage on two ranks, the ghost rows moved through the split entry points --------------------------------------------
FWD_NAMES = ("el", "er", "o", "op", "m", "den", "dpos")
BWD_NAMES = ("t", "der", "st", "del", "dz")


class Stages:
    """side A (dory_gatmh_bf16_ghosts on) and side B (off) of both ranks of the hub graph, everything else alike: the row-gather family
    with its bf16 forms, option gatmh_bf16_gather = v, the three switches of the contract.  The ghost rows travel as the rule makes
    them -- dory_halo_pack / dory_halo_unpack forward, dory_gatmh_bwd_pack / _unpack between the backward's phases -- by a device copy.
    lower: the option is set to 0 between the exchange and the aggregation that reads its rows (the readers of fp32 rows)"""

    def __init__(self, da, dims, heads, v, lower=False):
        import partition_oracle as po
        from halo_plan_ref import halo_plan
        self.da, self.dims, self.heads, self.v, self.lower = da, dims, heads, v, lower
        s, d, parts, rng = _hub_graph(2)
        V = len(parts)
        self.gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
        X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
        labels = rng.integers(0, dims[-1], V).astype(np.uint32)
        params = make_params(rng, dims, heads)
        self.A, self.B, self.plans = [], [], []
        for r, g in enumerate(self.gs):
            l2g = g["localToGlobal"]
            pl = halo_plan(g, parts, r, 2)
            for side, gh in ((self.A, 1), (self.B, 0)):
                ctx = make_gatmh(da, g, dims, heads, V, X[l2g], labels[l2g], params, {"gatmh_bf16_gather": v}, r, 2)
                ctx.gatmh_row_gather(1)
                ctx.gatmh_row_gather_bf16(1)
                for dd in (0, 1):
                    ctx.halo_plan(dd, pl[dd][0], pl[dd][1])
                _switches(ctx, gh)
                side.append(ctx)
            self.plans.append(pl)
            assert int(g["srcGhostCnt"]) and int(g["dstGhostCnt"])
        self.expect = dict(ZERO)

    def all(self):
        return self.A + self.B

    def option(self, v):
        for c in self.all():
            c.set_option("gatmh_bf16_gather", v)

    def move(self, side, dd, row_bytes, pack, unpack):
        import torch
        pl = self.plans
        n_send = [sum(len(x) for x in pl[r][dd][0]) for r in range(2)]
        n_recv = [sum(len(x) for x in pl[r][dd][1]) for r in range(2)]
        send = [torch.zeros(max(16, n_send[r] * row_bytes), dtype=torch.uint8, device="cuda") for r in range(2)]
        recv = [torch.zeros(max(16, n_recv[r] * row_bytes), dtype=torch.uint8, device="cuda") for r in range(2)]
        torch.cuda.synchronize()
        for r in range(2):
            pack(side[r], send[r].data_ptr())
            side[r].sync()
        for r in range(2):
            soff = np.concatenate([[0], np.cumsum([len(x) for x in pl[r][dd][0]])])
            for p in range(2):
                roff = np.concatenate([[0], np.cumsum([len(x) for x in pl[p][dd][1]])])
                n = len(pl[r][dd][0][p])
                recv[p][roff[r] * row_bytes:(roff[r] + n) * row_bytes] = send[r][soff[p] * row_bytes:(soff[p] + n) * row_bytes]
        torch.cuda.synchronize()
        for r in range(2):
            unpack(side[r], recv[r].data_ptr())
            side[r].sync()

    def same(self, l, names, what):
        for r in range(2):
            for nm in names:
                assert same_bits(self.A[r].download(l, nm), self.B[r].download(l, nm)), (what, "rank", r, "layer", l, nm)

    def check(self, where):
        for r in range(2):
            assert self.A[r].gatmh_bf16_ghosts_stats() == self.expect, (where, r, self.A[r].gatmh_bf16_ghosts_stats(), self.expect)
            sk = self.expect["twin_reads_rows"]
            assert self.A[r].halo_bf16_ghosts_stats()["conversions_skipped"] == sk, (where, r)
            assert self.B[r].gatmh_bf16_ghosts_stats() == ZERO and _stats(self.B[r]) == GHOST_ZERO, (where, r)

    def edge_pass(self, l):
        K, zw = _layer_shapes(self.dims, self.heads)[l]
        return not _dst_rowwise_covers(K, zw)

    def epoch(self):
        da, v, e = self.da, self.v, self.expect
        for l in range(2):
            for c in self.all():
                c.apply_vertex(l, da.FORWARD)
            for side in (self.A, self.B):
                eb, n = side[0].halo_wire_row(l + 1, da.FORWARD)
                assert eb == 2
                self.move(side, da.FORWARD, eb * n, lambda c, p: c.halo_pack(l + 1, da.FORWARD, p), lambda c, p: c.halo_unpack(l + 1, da.FORWARD, p))
            for c in self.all():
                c.apply_edge(l + 1, da.FORWARD)
            e["fwd_kept"] += 1
            e["scores_from_twin"] += 1
            self.check(("apply_edge", l))
            for r in range(2):
                assert self.A[r].halo_bf16_ghost_peek(l, "fg_z")[1] == hg.TWIN
            if self.lower:
                self.option(0)
            for c in self.all():
                c.aggregate(l + 1, da.FORWARD)
            self.option(v)
            e["widened" if self.lower else "twin_reads_rows"] += 1
            self.check(("forward", l))
            self.same(l, FWD_NAMES, "forward")
            self.same(*((l + 1, ("h",)) if l == 0 else (l, ("logits",))), "forward")
        for c in self.all():
            c.predict_gat(2)
        for l in (1, 0):
            for c in self.all():
                c.set_option("gatmh_bwd_phase", 1)
                c.aggregate(l + 1, da.BACKWARD)
            # (the edge pass gathers bf16 rows -- the twin -- iff this layer's forward ran the family's bf16 form; after a lowered forward it
            #  reads fg_z's fp32 rows, which that forward has widened already: state BOTH, nothing to count)
            if self.edge_pass(l) and not self.lower:
                e["twin_reads_rows"] += 1
            self.check(("phase 1", l))
            self.same(l, ("t", "der", "st"), "phase 1")
            for side in (self.A, self.B):
                R = side[0].gatmh_bwd_wire_row(l)[0]
                assert side[0].gatmh_bwd_wire_do(l)[0] == (2 if v == 2 else 4)
                self.move(side, da.BACKWARD, 4 * R, lambda c, p: c.gatmh_bwd_pack(l, p), lambda c, p: c.gatmh_bwd_unpack(l, p))
            if v == 2:
                e["bwd_kept_merged"] += 1
                for r in range(2):
                    assert self.A[r].halo_bf16_ghost_peek(l, "bg_do")[1] == hg.TWIN and self.A[r].halo_bf16_ghost_peek(l, "bg_st") == (None, hg.FP32)
            if self.lower:
                self.option(0)
            for c in self.all():
                c.set_option("gatmh_bwd_phase", 2)
                c.aggregate(l + 1, da.BACKWARD)
            self.option(v)
            if v == 2:
                e["widened" if self.lower else "twin_reads_rows"] += 1
            self.check(("phase 2", l))
            for c in self.all():
                c.apply_vertex(l, da.BACKWARD)
            self.same(l, BWD_NAMES, "backward")
            for r in range(2):
                for nm in ("a_l", "a_r", "w"):
                    assert same_bits(self.A[r].weight_grad_get(l, nm), self.B[r].weight_grad_get(l, nm)), ("grad", r, l, nm)
        for c in self.all():
            c.set_option("gatmh_bwd_phase", 0)
        # a download shows the same rounded rows on both sides
        for l in range(2):
            self.same(l, ("fg_z", "bg_do", "bg_st", "fg_el", "fg_er"), "ghost rows")

    def close(self):
        for c in self.all():
            c.close()


@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("dims,heads", [([24, 128, 6], [8, 1]), ([24, 96, 6], [3, 1]), ([16, 32, 5], [32, 1])])
def test_family_stage_by_stage_switch_on_against_off(da, dims, heads, v):
    """8 x 16 (scores from the gathered row), 3 x 32 (ld 96: el / fg_el gathered -- fg_el formed from the twin), 32 x 1 (the edge pass on the
    destination side); the ghost conversion is skipped on every bf16 pass and nothing is widened"""
    S = Stages(da, dims, heads, v)
    try:
        S.epoch()
        edge = sum(S.edge_pass(l) for l in range(2))
        assert S.expect == dict(ZERO, fwd_kept=2, scores_from_twin=2, bwd_kept_merged=2 * (v == 2), twin_reads_rows=2 + edge + 2 * (v == 2))
        for r in range(2):
            assert S.A[r].gatmh_row_gather_bf16_stats() == S.B[r].gatmh_row_gather_bf16_stats() == (2, edge, 2 * (v == 2))
    finally:
        S.close()


def test_readers_of_fp32_rows_find_the_twin_widened(da):
    """gatmh_bf16_gather lowered to 0 between the exchange and dory_aggregate, and again between the backward's phases: the fp32 forms of the
    family read fg_z / bg_do, the twins are widened first (counted), the bits are the switch-off run's.  Then a raw pointer: widened rows,
    state BOTH, and a later unpack is followed by a widening at once"""
    import torch
    S = Stages(da, [24, 128, 6], [8, 1], 2, lower=True)
    try:
        S.epoch()
        assert S.expect == dict(ZERO, fwd_kept=2, scores_from_twin=2, bwd_kept_merged=2, widened=4)
        c, d = S.A[0], S.da
        for r in range(2):
            for l in range(2):
                assert S.A[r].halo_bf16_ghost_peek(l, "fg_z")[1] == S.A[r].halo_bf16_ghost_peek(l, "bg_do")[1] == hg.BOTH
        tw, _ = _twin(c, 0, "fg_z")
        w0 = c.gatmh_bf16_ghosts_stats()["widened"]
        assert np.array_equal(_bits(_raw(c, 0, "fg_z")), _bits(hg.widen(tw)))             # (dory_tensor_info: BOTH already, nothing to widen)
        assert c.gatmh_bf16_ghosts_stats()["widened"] == w0
        eb, n = c.halo_wire_row(1, d.FORWARD)
        G = tw.shape[0]
        wire = np.zeros((G, n), np.uint16)
        wire[:, :128] = hb.round_bits(np.random.default_rng(3).uniform(-1, 1, (G, 128)).astype(np.float32))
        buf = torch.from_numpy(wire.view(np.int16).copy()).cuda()
        torch.cuda.synchronize()
        c.halo_unpack(1, d.FORWARD, buf.data_ptr())
        tw2, state = _twin(c, 0, "fg_z")
        assert state == hg.BOTH and not np.array_equal(tw2, tw)
        assert np.array_equal(_bits(_raw(c, 0, "fg_z")), _bits(hg.widen(tw2)))             # the raw rows followed the twin
        assert c.gatmh_bf16_ghosts_stats()["widened"] == w0                             # (the exchange's own widening is not a reader's)
    finally:
        S.close()


# ---- 4 / 5 / 7. whole epochs over the in-process transport (and the scatter transport) ----------------------------------------------------
DIMS, HEADS, ZW = [20, 128, 6], [8, 1], [128, 6]
DL = [(l, nm) for l in range(2) for nm in ("z", "el", "er", "o", "op", "m", "den", "dpos", "t", "del", "der", "dz", "do", "st")] + [(1, "logits"), (1, "h")]
GHOST_DL = [(l, nm) for l in range(2) for nm in ("fg_z", "fg_el", "bg_do", "bg_st")]


def _drive(da, case, gh, family, merged=0, fused=0, opts=None, epochs=2, halo16=1, mode=2, transport="local", gh_of=None):
    """the ranks of a golden partitioning, a host thread each, epochs driven call by call as tests/test_gpu_gatmh_halo_bf16.py::_drive does
    (the sweep forms' last layer -- one head of 6 -- runs its backward with gatmh_bf16_gather = 1; the ranks meet at a barrier after every
    change of the option).  family: the row-gather kernels with their bf16 forms in place of the sweep forms.  Returns downloads, weights,
    gradients and the counters of every rank before (`kept`) and after (`after`) the downloads"""
    pobjs, parts = _golden(da, case)
    P, V = len(pobjs), len(parts)
    rng = np.random.default_rng(31)
    X = rng.uniform(-1, 1, (V, DIMS[0])).astype(np.float32)
    labels = rng.integers(0, DIMS[-1], V).astype(np.uint32)
    inw = [DIMS[0], ZW[0]]
    Ws = [(rng.standard_normal((inw[l], ZW[l])) / np.sqrt(inw[l])).astype(np.float32) for l in range(2)]
    Al = [(rng.standard_normal(ZW[l]) * 0.3).astype(np.float32) for l in range(2)]
    Ar = [(rng.standard_normal(ZW[l]) * 0.3).astype(np.float32) for l in range(2)]
    bwd_value = [mode if family or backward_takes_the_sweep_forms(HEADS[l], ZW[l] // HEADS[l]) else min(mode, 1) for l in range(2)]
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
        if family:
            ctx.gatmh_row_gather(1)
            ctx.gatmh_row_gather_bf16(1)
        ctx.halo_fused_pack(fused)
        ctx.halo_fused_pack_bf16(fused)
        ctx.gatmh_bwd_merged_exchange(merged)
        _switches(ctx, gh if gh_of is None else gh_of[r], halo16)
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
        ctxs[r].set_option("gatmh_bf16_gather", v)
        bar.wait(30)

    def rank(r):
        c = ctxs[r]
        try:
            for _ in range(epochs):
                value(r, mode)
                for l in range(2):
                    c.apply_vertex(l, da.FORWARD)
                    c.halo_exchange(l + 1, da.FORWARD)
                    c.apply_edge(l + 1, da.FORWARD)
                    c.aggregate(l + 1, da.FORWARD)
                c.predict_gat(2)
                for l in (1, 0):
                    value(r, bwd_value[l])
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

    def counters(c):
        return {"gh": c.gatmh_bf16_ghosts_stats(), "ghosts": c.halo_bf16_ghosts_stats(), "bf16": c.halo_bf16_rows_stats(),
                "merged": c.gatmh_bwd_merged_exchange_stats(), "direct": c.get_option("halo_direct_recvs"), "staged": c.get_option("halo_staged_recvs"),
                "rows16": c.gatmh_row_gather_bf16_stats(), "gathers": (c.get_option("gatmh_bf16_gathers_fwd"), c.get_option("gatmh_bf16_gathers_src")),
                "states": {(l, nm): c.halo_bf16_ghost_peek(l, nm)[1] for l in range(2) for nm in ("fg_z", "bg_do", "bg_st", "fg_el", "fg_er")}}
    out = {"errors": errors, "views": _own_views(pobjs), "tensors": [], "ghost_rows": [], "weights": [], "wgrads": [], "kept": [], "after": [],
           "bwd_value": bwd_value}
    if not any(errors):
        for r, c in enumerate(ctxs):
            vw = out["views"][r]
            N, Gs, Gd = int(vw["localVtxCnt"]), int(vw["srcGhostCnt"]), int(vw["dstGhostCnt"])
            out["kept"].append(counters(c))
            skip = lambda nm: (nm in ("fg_z", "fg_el") and not Gs) or (nm in ("bg_do", "bg_st") and not Gd)
            out["tensors"].append({(l, nm): c.download(l, nm) for (l, nm) in DL} if N else {})
            out["ghost_rows"].append({(l, nm): c.download(l, nm) for (l, nm) in GHOST_DL if not skip(nm)} if N else {})
            out["weights"].append([{nm: c.weight_get(l, nm) for nm in ("w", "a_l", "a_r")} for l in range(2)])
            out["wgrads"].append([{nm: c.weight_grad_get(l, nm) for nm in ("w", "a_l", "a_r")} for l in range(2)])
            out["after"].append(counters(c))
    for c in ctxs:
        c.sync()
    for c in ctxs:
        c.close()
    for p in pobjs:
        p.close()
    return out


def _equal(a, b, what, ghost_rows=True):
    assert not any(a["errors"]) and not any(b["errors"]), (what, a["errors"], b["errors"])
    for r in range(len(a["tensors"])):
        for part in ("tensors",) + (("ghost_rows",) if ghost_rows else ()):
            assert set(a[part][r]) == set(b[part][r]), (what, r, part)
            for k in a[part][r]:
                assert same_bits(a[part][r][k], b[part][r][k]), (what, r, k)
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                assert same_bits(a["weights"][r][l][nm], b["weights"][r][l][nm]), (what, r, l, nm, "W")
                assert same_bits(a["wgrads"][r][l][nm], b["wgrads"][r][l][nm]), (what, r, l, nm, "dW")


def _live_with_ghosts(run):
    return [r for r, g in enumerate(run["views"]) if int(g["localVtxCnt"]) and int(g["srcGhostCnt"]) and int(g["dstGhostCnt"])]


def _check_off(off, what):
    for r, k in enumerate(off["after"]):
        assert k["gh"] == ZERO and {x: k["ghosts"][x] for x in GHOST_ZERO} == GHOST_ZERO and k["ghosts"]["twin_bytes"] == 0, (what, r, k)
        assert set(k["states"].values()) == {hg.FP32}, (what, r, k["states"])


@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty"])
def test_family_epochs_switch_on_equals_switch_off(da, case):
    """two epochs, the row-gather family, gatmh_bf16_gather = 2 (per epoch five bf16 passes with ghost rows: two forwards, the edge pass on the
    destination side of the last layer -- one head of 6 --, two source sides): merged exchange off / on times fused pack off / on, once with exact rows,
    once with a plan made with halo_direct_recv = 1 (rows land in the twins themselves: no keep kernel)"""
    E = 2
    for merged in (0, 1):
        for fused in (0, 1):
            what = (case, "merged", merged, "fused", fused)
            off = _drive(da, case, 0, True, merged, fused)
            on = _drive(da, case, 1, True, merged, fused)
            _equal(off, on, what)
            _check_off(off, what)
            live = _live_with_ghosts(on)
            assert len(live) >= 2
            for r in live:
                k, a = on["kept"][r], on["after"][r]
                assert k["gh"] == dict(ZERO, fwd_kept=2 * E, scores_from_twin=2 * E, twin_reads_rows=5 * E,
                                       bwd_kept=0 if merged else 2 * E, bwd_kept_merged=2 * E if merged else 0), (what, r, k["gh"])
                assert k["ghosts"]["landed_by_kernel"] == 4 * E and k["ghosts"]["landed_direct"] == 0 and k["ghosts"]["conversions_skipped"] == 5 * E
                assert k["ghosts"]["twin_bytes"] > 0 and k["ghosts"]["widened"] == 0, (what, r, k["ghosts"])
                assert k["states"] == {(l, nm): (hg.TWIN if nm in ("fg_z", "bg_do") else hg.FP32) for (l, nm) in k["states"]}
                assert a["gh"]["widened"] == 4 and a["ghosts"]["widened"] == 4                  # the downloads of fg_z / bg_do of both layers
                assert k["merged"][0] == (2 * E if merged else 0) and k["rows16"] == off["kept"][r]["rows16"] == (2 * E, E, 2 * E)
                assert k["bf16"] == off["kept"][r]["bf16"], (what, r)                        # the same bytes on the wire
            for r in set(range(len(on["views"]))) - set(live):                               # a rank without ghosts reads no twin
                g = on["kept"][r]["gh"]
                assert g["twin_reads_rows"] == g["scores_from_twin"] == g["widened"] == 0, (what, r, g)
    # exact rows: layer 1 ships 8 elements into an ld of 32
    what = (case, "halo_exact_rows")
    off = _drive(da, case, 0, True, 1, 1, {"halo_exact_rows": 1})
    on = _drive(da, case, 1, True, 1, 1, {"halo_exact_rows": 1})
    _equal(off, on, what)
    _check_off(off, what)
    for r in _live_with_ghosts(on):
        assert on["kept"][r]["gh"]["twin_reads_rows"] == 5 * E and on["kept"][r]["ghosts"]["landed_by_kernel"] == 4 * E, (what, r)
    # a direct plan: this switch turns its wire from fp32 to bf16 (the switch-off run ships fp32 rows: its fg_z / fg_el hold unrounded
    # rows, which no kernel of the family reads at these shapes), and the rows land in the twins themselves
    what = (case, "halo_direct_recv")
    off = _drive(da, case, 0, True, 1, 1, {"halo_direct_recv": 1})
    on = _drive(da, case, 1, True, 1, 1, {"halo_direct_recv": 1})
    _equal(off, on, what, ghost_rows=False)
    _check_off(off, what)
    for r in _live_with_ghosts(on):
        k = on["kept"][r]
        assert k["gh"] == dict(ZERO, fwd_kept=2 * E, scores_from_twin=2 * E, twin_reads_rows=5 * E, bwd_kept=2 * E), (what, r, k["gh"])
        assert k["ghosts"]["landed_direct"] == 4 * E and k["ghosts"]["landed_by_kernel"] == 0, (what, r, k["ghosts"])
        assert k["merged"][0] == 0 and off["kept"][r]["bf16"][0] == 0 and k["bf16"][0] == 4 * E, (what, r, k)
    for r, g in enumerate(on["views"]):                                                      # the ghost rows: the fp32 run's, rounded
        for l in range(2):
            if (l, "fg_z") in on["ghost_rows"][r]:
                assert same_bits(on["ghost_rows"][r][(l, "fg_z")], hb.rounded(off["ghost_rows"][r][(l, "fg_z")])), (what, r, l)
                assert same_bits(on["ghost_rows"][r][(l, "bg_do")], hb.rounded(off["ghost_rows"][r][(l, "bg_do")])), (what, r, l)


def test_sweep_forms_read_the_twin_and_the_finish_kernel_widens(da):
    """parts_toy60_p2, 8 x 16 then one head of 6, the sweep forms (spmm_blk_nb = 8): the same equality; the bf16 passes skip the conversion
    of the ghost rows (both forwards, the source side of layer 0); the finish kernel of every forward reads fg_z's fp32 rows: a widening"""
    case, E = "parts_toy60_p2", 2
    off = _drive(da, case, 0, False, 1, 1)
    on = _drive(da, case, 1, False, 1, 1)
    assert on["bwd_value"] == [2, 1]
    _equal(off, on, "sweeps")
    _check_off(off, "sweeps")
    for r in _live_with_ghosts(on):
        k = on["kept"][r]
        assert k["gathers"] == off["kept"][r]["gathers"] == (2 * E, E) and k["rows16"] == (0, 0, 0), (r, k)
        assert k["gh"] == dict(ZERO, fwd_kept=2 * E, scores_from_twin=2 * E, twin_reads_sweep=3 * E, bwd_kept_merged=E, widened=2 * E), (r, k["gh"])
        assert k["ghosts"]["conversions_skipped"] == 3 * E and k["ghosts"]["widened"] == 2 * E, (r, k["ghosts"])
        assert k["bf16"] == off["kept"][r]["bf16"], r


def test_inert_cases_leave_the_twins_untouched(da):
    """the switch on without dory_gatmh_halo_bf16, with gatmh_bf16_gather = 0, and over the scatter transport: the twins exist, nothing
    lands in them, no counter moves, the wire carries the same bytes, and every result is the switch-off run's"""
    case = "parts_toy60_p2"
    for what, kw in (("without dory_gatmh_halo_bf16", dict(family=True, halo16=0)), ("gatmh_bf16_gather = 0", dict(family=True, mode=0)),
                     ("the scatter transport", dict(family=True, transport="scatter"))):
        off = _drive(da, case, 0, merged=1, fused=1, **kw)
        on = _drive(da, case, 1, merged=1, fused=1, **kw)
        _equal(off, on, what)
        _check_off(off, what)
        for r in range(2):
            k = on["after"][r]
            assert k["gh"] == ZERO and {x: k["ghosts"][x] for x in GHOST_ZERO} == GHOST_ZERO and k["ghosts"]["twin_bytes"] > 0, (what, r, k)
            assert set(k["states"].values()) == {hg.FP32} and k["bf16"] == off["after"][r]["bf16"] and k["bf16"][0] == 0, (what, r, k)


# ---- 8. refusals ---------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_switch_underneath(da):
    for gnn, dims in ((da.GCN, [4, 41, 2]), (da.GAT, [4, 16, 2])):
        c = da.Context(0)
        with pytest.raises(da.DoryError, match="error -1.*gatmh_bf16_ghosts"):
            c.gatmh_bf16_ghosts(1)                                          # before dory_configure
        c.configure(gnn, dims, 100, 0, 2)
        for on in (0, 1):
            with pytest.raises(da.DoryError, match="error -1.*gatmh_bf16_ghosts.*DORY_GATMH"):
                c.gatmh_bf16_ghosts(on)
        c.close()
    c = da.Context(0)
    c.configure(da.GATMH, [16, 32, 8], 100, 0, 2)
    with pytest.raises(da.DoryError, match="error -1.*gatmh_bf16_ghosts.*dory_preallocate"):
        c.gatmh_bf16_ghosts(1)
    c.close()
    ctx = _rank0_of_2(da, [12, 32, 3], [4, 1], 7, 1)
    try:
        assert ctx.gatmh_bf16_ghosts_stats() == ZERO
        for on in (0, 1):
            with pytest.raises(da.DoryError, match="error -1.*gatmh_bf16_ghosts.*dory_halo_bf16_ghosts is off"):
                ctx.gatmh_bf16_ghosts(on)
        ctx.halo_bf16_ghosts(1)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0 and ctx.halo_bf16_ghost_peek(0, "fg_z") == (None, hg.FP32)      # inert for this model
        for bad in (-1, 2, 7):
            with pytest.raises(da.DoryError, match="error -1.*gatmh_bf16_ghosts.*0 or 1"):
                ctx.gatmh_bf16_ghosts(bad)
        ctx.gatmh_bf16_ghosts(1)
        want = sum(2 * 7 * hx.pad_ld(w) for w in (32, 3)) * 2                   # fg_z and bg_do of both layers: rows x ld x 2 bytes
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == want
        for l in range(2):
            assert ctx.halo_bf16_ghost_peek(l, "fg_z")[0] and ctx.halo_bf16_ghost_peek(l, "bg_do")[0]
            for nm in ("bg_st", "fg_el", "fg_er"):
                assert ctx.halo_bf16_ghost_peek(l, nm) == (None, hg.FP32), (l, nm)
        ctx.gatmh_bf16_ghosts(1)                                            # again: nothing new
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == want
        ctx.gatmh_bf16_ghosts(0)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0
        ctx.gatmh_bf16_ghosts(1)
        # dory_halo_bf16_ghosts(0) clears this switch and frees its twins; turning it on again does not bring them back
        ctx.halo_bf16_ghosts(0)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0 and ctx.halo_bf16_ghost_peek(0, "fg_z") == (None, hg.FP32)
        ctx.halo_bf16_ghosts(1)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0
        ctx.gatmh_bf16_ghosts(1)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == want and ctx.gatmh_bf16_ghosts_stats() == ZERO
    finally:
        ctx.close()
    # inside a recording (a single partition: an epoch graph records no other)
    from test_gpu_gatmh_bf16_gather import hub_graph
    dims, heads = [24, 32, 8], [4, 2]
    g, rng = hub_graph(dims, 200, 1500)
    X = rng.uniform(-1, 1, (200, dims[0])).astype(np.float32)
    one = make_gatmh(da, g, dims, heads, 200, X, rng.integers(0, 8, 200).astype(np.uint32), make_params(rng, dims, heads), {"spmm_blk_nb": 8})
    try:
        _switches(one, 1)
        one.epoch_graph_begin()
        for on in (0, 1):
            with pytest.raises(da.DoryError, match="error -1.*gatmh_bf16_ghosts.*recorded"):
                one.gatmh_bf16_ghosts(on)
        one.epoch_graph_drop()
        one.gatmh_bf16_ghosts(0)
    finally:
        one.close()


def test_local_ranks_that_disagree_fail_before_anything_is_enqueued(da):
    case = "parts_toy60_p2"
    bad = _drive(da, case, 1, True, gh_of=[1, 0], epochs=1)
    assert all(e is not None for e in bad["errors"]), bad["errors"]
    assert any("error -4" in str(e) and "dory_gatmh_bf16_ghosts differs" in str(e) for e in bad["errors"]), bad["errors"]
    # one pair of contexts, stage by stage: refused, set right, then the exchange goes through
    pobjs, parts = _golden(da, case)
    ctxs = []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, DIMS, len(parts), r, 2)
        ctx.gatmh_heads(HEADS)
        for k, v in (("spmm_blk_nb", 8), ("local_timeout_ms", 300), ("gatmh_bf16_gather", 2)):
            ctx.set_option(k, v)
        part.upload(ctx, parts)
        ctx.preallocate()
        g = part.view()
        ctx.fill_uniform(0, "h", 3, -1.0, 1.0, g["localToGlobal"])
        ctx.labels_upload(np.zeros(int(g["localVtxCnt"]), np.uint32))
        ctx.weights_init_xavier()
        _switches(ctx, 1 - r)
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    for c in ctxs:
        c.apply_vertex(0, da.FORWARD)
    for r in (0, 1):
        with pytest.raises(da.DoryError, match=r"error -4.*dory_gatmh_bf16_ghosts differs"):
            ctxs[r].halo_exchange(1, da.FORWARD)
        assert ctxs[r].gatmh_bf16_ghosts_stats() == ZERO and ctxs[r].halo_bf16_rows_stats() == (0, 0, 0)
    ctxs[1].gatmh_bf16_ghosts(1)
    for c in ctxs:
        c.halo_exchange(1, da.FORWARD)
    for c in ctxs:
        c.apply_edge(1, da.FORWARD)
        c.aggregate(1, da.FORWARD)
        c.sync()
        s = c.gatmh_bf16_ghosts_stats()
        assert s["fwd_kept"] == 1 and s["scores_from_twin"] == 1 and s["twin_reads_sweep"] == 1, s
    for c in ctxs:
        c.close()
    for p in pobjs:
        p.close()


# ---- 9. the epoch graph ---------------------------------------------------------------------------------------------------------------------
def test_recorded_epochs_equal_eager_epochs_with_every_switch_on(da):
    """a single partition (an epoch graph records no exchange): an eager epoch, then recorded ones, are bit for bit what eager epochs
    compute; the shadow rows the eager epoch reserved are enough inside the recording"""
    from test_gpu_gatmh_bf16_gather import hub_graph
    dims, heads = [24, 64, 6], [4, 1]
    states = []
    for graph in (0, 1):
        g, rng = hub_graph(dims, 300, 4000)
        X = rng.uniform(-1, 1, (300, dims[0])).astype(np.float32)
        labels = rng.integers(0, dims[-1], 300).astype(np.uint32)
        ctx = make_gatmh(da, g, dims, heads, 300, X, labels, make_params(rng, dims, heads), {})
        ctx.gatmh_row_gather(1)
        ctx.gatmh_row_gather_bf16(1)
        ctx.set_option("gatmh_bf16_gather", 2)
        _switches(ctx, 1)
        ctx.adam_config(0.01)
        ctx.set_option("epoch_graph", graph)
        eng = da.NativeEngine(ctx)
        eng.run(3)
        eng.run(2)
        if graph:
            assert ctx.get_option("epoch_graph_recorded") == 1
        assert ctx.gatmh_bf16_ghosts_stats() == ZERO and ctx.gatmh_row_gather_bf16_stats()[0] == (4 if graph else 10)
        st = {}
        for l in range(2):
            for nm in ("w", "a_l", "a_r"):
                st[(nm, l)] = ctx.weight_get(l, nm)
                st[("d" + nm, l)] = ctx.weight_grad_get(l, nm)
            for nm in ("z", "o", "op", "m", "den", "dz", "el", "t", "der", "del"):
                st[(nm, l)] = ctx.download(l, nm)
        states.append(st)
        eng.close()
        ctx.close()
    for k in states[0]:
        assert same_bits(states[0][k], states[1][k]), k
