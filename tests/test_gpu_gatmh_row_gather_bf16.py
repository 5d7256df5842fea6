"""dory_gatmh_row_gather_bf16 (include/dorylus_hip.h): option gatmh_bf16_gather on the multi-head GAT's row-gather kernels
(csrc/gat_mh_rows.hip).  The bf16 kernels share their fp32 siblings' bodies and differ in the gathered chunk alone (one 8-byte load of
four bf16 from the shadow rows, widened exactly), so the contract is bit equality with the fp32 family on rows rounded beforehand.

The scheme of tests/test_gpu_gatmh_bf16_gather.py, stage by stage through the C-ABI, on every rank of a run:
  context A: gatmh_row_gather(1), gatmh_row_gather_bf16(1), gatmh_bf16_gather = v;   context B: gatmh_row_gather(1), bf16 off.
  B's z / fg_z are rounded on the host (nearest even) between apply_edge and aggregate(FORWARD) -- and kept rounded through the
  backward's phase 1 on layers whose destination side is the edge pass, which gathers them again --, then restored; for v = 2 B's
  do / bg_do are rounded between the phases 1 and 2.
Asserted bit for bit: o, op, m, den, dpos, the next h / logits, t, der, st, del, dz and the gradients of a_l / a_r / w; the counters
moved by exactly the passes expected and B's did not move."""
import numpy as np
import pytest

from test_gpu_gatmh_bf16_gather import bf16, counters, make_gatmh, make_params, same_bits, special_rows
from test_gpu_gatmh_row_gather import _dst_rowwise_covers, _hub_graph, _layer_shapes

pytestmark = pytest.mark.gpu

FWD_NAMES = ("o", "op", "m", "den", "dpos")
BWD_NAMES = ("t", "der", "st", "del", "dz")
# the smallest set that reaches every instantiation: one per GROUP x HPQ, both ELFLY arms
SHAPES = [([24, 32, 8], [4, 2]), ([24, 64, 6], [4, 1]), ([24, 128, 6], [8, 1]), ([24, 256, 6], [4, 1]), ([24, 256, 9], [32, 1]),
          ([24, 64, 6], [32, 1]),       # D = 2
          ([16, 32, 5], [32, 1]),       # D = 1: two rows in flight on the source side, destination-side edge pass
          ([12, 100, 6], [1, 1]),
          ([24, 96, 6], [3, 1]), ([24, 160, 5], [5, 1])]     # rows whose float4 count is no power of two: el is gathered
DIMS8, HEADS8 = [24, 128, 6], [8, 1]


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def bf16_stats(ctx):
    return ctx.gatmh_row_gather_bf16_stats()


class Ranks:
    """contexts A and B of every rank of a P-way split (P = 1: one partition), the ghost rows moved by halo_pack_tensor /
    halo_unpack_tensor and a device copy as in tests/test_gpu_gatmh_row_gather.py::_partitioned"""

    def __init__(self, da, gs, parts, X, labels, params, dims, heads, v, opts=None, mode=1, plant=None, representable=False):
        from halo_plan_ref import halo_plan
        self.da, self.v, self.P, self.dims, self.heads = da, v, len(gs), dims, heads
        self.plant, self.representable = plant, representable
        self.gs, self.A, self.B, self.plans = gs, [], [], []
        V = len(parts)
        for r, g in enumerate(gs):
            l2g = g["localToGlobal"]
            for side in (self.A, self.B):
                ctx = make_gatmh(da, g, dims, heads, V, X[l2g], labels[l2g], params, opts, r, self.P)
                ctx.gatmh_row_gather(mode)
                side.append(ctx)
            self.A[r].gatmh_row_gather_bf16(1)
            self.A[r].set_option("gatmh_bf16_gather", v)
            pl = halo_plan(g, parts, r, self.P) if self.P > 1 else None
            if pl:
                for ctx in (self.A[r], self.B[r]):
                    for dd in (0, 1):
                        ctx.halo_plan(dd, pl[dd][0], pl[dd][1])
            self.plans.append(pl)
        self.live = [r for r, g in enumerate(gs) if int(g["localVtxCnt"])]
        # (gatmh_sweep = 0 at dory_preallocate: no per-layer record of a forward that left op / dpos -- every destination side is an edge pass)
        self.rowwise = (opts or {}).get("gatmh_sweep", 1) != 0
        self.expect = [[0, 0, 0] for _ in gs]          # A's bf16 passes: forward, destination-side edge pass, source side

    def all(self):
        return self.A + self.B

    def exchange(self, ctxs, layer, src_name, ghost_name, dd):
        import torch
        P, plans = self.P, self.plans
        if P == 1:
            return
        _, _, ld, _ = ctxs[0].info(layer, src_name)
        send = [torch.zeros(max(1, sum(len(x) for x in plans[r][dd][0])) * ld, device="cuda") for r in range(P)]
        recv = [torch.zeros(max(1, sum(len(x) for x in plans[r][dd][1])) * ld, device="cuda") for r in range(P)]
        torch.cuda.synchronize()
        for r in range(P):
            ctxs[r].halo_pack_tensor(layer, src_name, dd, send[r].data_ptr())
            ctxs[r].sync()
        for r in range(P):
            soff = np.concatenate([[0], np.cumsum([len(x) for x in plans[r][dd][0]])])
            for p in range(P):
                roff = np.concatenate([[0], np.cumsum([len(x) for x in plans[p][dd][1]])])
                n = len(plans[r][dd][0][p])
                recv[p][roff[r] * ld:(roff[r] + n) * ld] = send[r][soff[p] * ld:(soff[p] + n) * ld]
        torch.cuda.synchronize()
        for r in range(P):
            ctxs[r].halo_unpack_tensor(layer, ghost_name, dd, recv[r].data_ptr())
            ctxs[r].sync()

    def ghosts(self, r, name):
        return int(self.gs[r]["srcGhostCnt" if name == "fg_z" else "dstGhostCnt"])

    def round_in_b(self, l, local, ghost):
        """B's rows of `local` / `ghost` rounded on the host; returns what restores them"""
        kept = []
        for r in self.live:
            for nm in (local, ghost):
                if nm == ghost and not self.ghosts(r, ghost):
                    continue
                t = self.B[r].download(l, nm)
                kept.append((r, nm, t))
                self.B[r].upload(l, nm, bf16(t))
        return kept

    def restore(self, l, kept):
        for r, nm, t in kept:
            self.B[r].upload(l, nm, t)

    def same(self, l, names, what):
        for r in self.live:
            for nm in names:
                assert same_bits(self.A[r].download(l, nm), self.B[r].download(l, nm)), (what, "rank", r, "layer", l, nm)

    def check_counters(self, where):
        for r in range(self.P):
            a = bf16_stats(self.A[r])
            assert a == tuple(self.expect[r]), (where, r, a, self.expect[r])
            assert counters(self.A[r]) == (self.expect[r][0], self.expect[r][2]), (where, r, counters(self.A[r]))
            rows = self.A[r].gatmh_row_gather_stats()
            assert rows[0] >= a[0] and rows[1] >= a[1] and rows[3] >= a[2], (where, r, rows, a)      # (those passes are counted there too)
            assert bf16_stats(self.B[r]) == (0, 0, 0) and counters(self.B[r]) == (0, 0), (where, r)

    def edge_pass(self, l):
        K, zw = _layer_shapes(self.dims, self.heads)[l]
        return not (self.rowwise and _dst_rowwise_covers(K, zw))

    def epoch(self):
        da, L = self.da, 2
        rounded_z = {}
        for l in range(L):
            for c in self.all():
                c.apply_vertex(l, da.FORWARD)
            if self.plant is not None or self.representable:
                for r in self.live:
                    z = self.B[r].download(l, "z")
                    z = self.plant(z) if self.plant is not None else z
                    z = bf16(z) if self.representable else z
                    self.A[r].upload(l, "z", z)
                    self.B[r].upload(l, "z", z)
            self.exchange(self.A, l, "z", "fg_z", da.FORWARD)
            self.exchange(self.B, l, "z", "fg_z", da.FORWARD)
            for c in self.all():
                c.apply_edge(l + 1, da.FORWARD)
            kept = self.round_in_b(l, "z", "fg_z")
            for c in self.all():
                c.aggregate(l + 1, da.FORWARD)
            for r in self.live:
                self.expect[r][0] += 1
            self.check_counters(("forward", l))
            if self.edge_pass(l):
                rounded_z[l] = kept
            else:
                self.restore(l, kept)
            self.same(l, FWD_NAMES, "forward")
            self.same(*((l + 1, ("h",)) if l < L - 1 else (l, ("logits",))), "forward")
        for c in self.all():
            c.predict_gat(L)
        for l in range(L - 1, -1, -1):
            for c in self.all():
                c.set_option("gatmh_bwd_phase", 1)
                c.aggregate(l + 1, da.BACKWARD)
            if l in rounded_z:
                self.restore(l, rounded_z[l])
                for r in self.live:
                    self.expect[r][1] += 1
            self.check_counters(("phase 1", l))
            self.same(l, ("t", "der", "st"), "phase 1")
            if self.representable:
                for r in self.live:
                    do = bf16(self.B[r].download(l, "do"))
                    self.A[r].upload(l, "do", do)
                    self.B[r].upload(l, "do", do)
            for side in (self.A, self.B):
                self.exchange(side, l, "do", "bg_do", da.BACKWARD)
                self.exchange(side, l, "st", "bg_st", da.BACKWARD)
            kept = self.round_in_b(l, "do", "bg_do") if self.v >= 2 else []
            for c in self.all():
                c.set_option("gatmh_bwd_phase", 2)
                c.aggregate(l + 1, da.BACKWARD)
            self.restore(l, kept)
            if self.v >= 2:
                for r in self.live:
                    self.expect[r][2] += 1
            self.check_counters(("phase 2", l))
            for c in self.all():
                c.apply_vertex(l, da.BACKWARD)
            self.same(l, BWD_NAMES, "backward")
            for r in self.live:
                for nm in ("a_l", "a_r", "w"):
                    assert same_bits(self.A[r].weight_grad_get(l, nm), self.B[r].weight_grad_get(l, nm)), ("grad", r, l, nm)
        for c in self.all():
            c.set_option("gatmh_bwd_phase", 0)

    def close(self):
        for c in self.all():
            c.close()


def _inputs(rng, V, dims, heads):
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    return X, labels, make_params(rng, dims, heads)


def _hub_ranks(da, P, dims, heads, v, **kw):
    import partition_oracle as po
    s, d, parts, rng = _hub_graph(P)
    V = len(parts)
    gs = [po.preprocess(s, d, parts if P > 1 else np.zeros(V, np.int64), r, P) for r in range(P)]
    X, labels, params = _inputs(rng, V, dims, heads)
    return Ranks(da, gs, parts, X, labels, params, dims, heads, v, **kw)


# ---- 1. A against B over every instantiation, one partition and two ranks -----------------------------------------------------------
@pytest.mark.parametrize("v", [1, 2])
@pytest.mark.parametrize("P", [1, 2])
@pytest.mark.parametrize("dims,heads", SHAPES)
def test_bf16_passes_equal_fp32_passes_on_rounded_rows(da, dims, heads, P, v):
    R = _hub_ranks(da, P, dims, heads, v)
    try:
        R.epoch()
        edge = sum(R.edge_pass(l) for l in range(2))
        for r in R.live:
            assert bf16_stats(R.A[r]) == (2, edge, 2 if v == 2 else 0), (r, bf16_stats(R.A[r]))
            assert R.A[r].gatmh_row_gather_stats() == (2, edge, 2 - edge, 2)
    finally:
        R.close()


def test_planted_ties_binade_edges_and_subnormals(da):
    rng = np.random.default_rng(9)
    R = _hub_ranks(da, 2, DIMS8, HEADS8, 2, plant=lambda z: special_rows(rng, z))
    try:
        R.epoch()
    finally:
        R.close()


@pytest.mark.parametrize("dims,heads", [(DIMS8, HEADS8), ([16, 32, 5], [32, 1])])
def test_identity_on_bf16_representable_rows(da, dims, heads):
    """z and do hold bf16-representable values in both contexts: v = 2 and v = 0 give the same bits (B's rounding changes nothing)"""
    R = _hub_ranks(da, 2, dims, heads, 2, representable=True)
    try:
        R.epoch()
    finally:
        R.close()


# ---- 2. the edges of the row walk ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [5, 67])
def test_rows_without_edges_and_odd_row_counts(da, N):
    """the graph of tests/test_gpu_gatmh_row_gather.py: vertex 0 has no in-edges, vertex 1 no out-edges, N no multiple of a block's rows"""
    import partition_oracle as po
    rng = np.random.default_rng(N)
    E = 6 * N
    s, d = rng.integers(1, N, E), rng.integers(1, N, E)
    s[s == 1] = 2
    s[:3] = 0
    g = po.preprocess(s, d, np.zeros(N, np.int64), 0, 1)
    assert g["colPtr"][1] == g["colPtr"][0] and g["rowPtr"][2] == g["rowPtr"][1]
    X, labels, params = _inputs(rng, N, DIMS8, HEADS8)
    R = Ranks(da, [g], np.zeros(N, np.int64), X, labels, params, DIMS8, HEADS8, 2)
    try:
        R.epoch()
        for l in range(2):
            assert np.array_equal(R.A[0].download(l, "o")[0], bf16(R.A[0].download(l, "z")[0])), l       # (the self edge's row is a rounded row too)
            assert np.all(R.A[0].download(l, "den")[0] == 1.0), l
    finally:
        R.close()


def test_ghosts_on_one_side_only(da):
    """every cross edge runs from rank 0 to rank 1: rank 0 has no ghost sources (a null fg_z), rank 1 no ghost destinations (a null bg_do)"""
    import partition_oracle as po
    rng = np.random.default_rng(4)
    V, E = 80, 700
    parts = (np.arange(V) >= 40).astype(np.int64)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    back = (parts[s] == 1) & (parts[d] == 0)
    d[back] = rng.integers(40, V, int(back.sum()))
    gs = [po.preprocess(s, d, parts, r, 2) for r in range(2)]
    assert gs[0]["srcGhostCnt"] == 0 and gs[0]["dstGhostCnt"] > 0 and gs[1]["srcGhostCnt"] > 0 and gs[1]["dstGhostCnt"] == 0
    X, labels, params = _inputs(rng, V, DIMS8, HEADS8)
    R = Ranks(da, gs, parts, X, labels, params, DIMS8, HEADS8, 2)
    try:
        R.epoch()
    finally:
        R.close()


# ---- 3. the dispatch ------------------------------------------------------------------------------------------------------------------
def test_mode_0_fall_back_runs_where_it_is_refused_with_the_switch_off(da):
    """two ranks, gatmh_sweep = 0, gatmh_blocked = 0, mode 0: the partitioned call falls back to the family; v = 2 runs with the switch
    on (A against B as above) and is refused with it off, with the message as before"""
    opts = {"gatmh_sweep": 0, "gatmh_blocked": 0}
    R = _hub_ranks(da, 2, [24, 64, 6], [4, 1], 2, opts=opts, mode=0)
    try:
        R.epoch()
        for r in R.live:
            assert bf16_stats(R.A[r])[0] == 2 and bf16_stats(R.A[r])[2] == 2, (r, bf16_stats(R.A[r]))
        # the same call with the switch off
        c = R.A[0]
        c.gatmh_row_gather_bf16(0)
        before = bf16_stats(c), c.gatmh_row_gather_stats()
        with pytest.raises(da.DoryError, match="needs the sweep form of the forward pass.*gatmh_sweep = 0"):
            c.aggregate(1, da.FORWARD)
        with pytest.raises(da.DoryError, match="needs the sweep forms of the backward pass.*gatmh_sweep = 0"):
            c.aggregate(2, da.BACKWARD)
        assert (bf16_stats(c), c.gatmh_row_gather_stats()) == before
    finally:
        R.close()


def _single(da, dims, heads, V, E, opts, seed=5):
    from test_gpu_gatmh_bf16_gather import hub_graph
    g, rng = hub_graph(dims, V, E)
    X, labels, params = _inputs(rng, V, dims, heads)
    return make_gatmh(da, g, dims, heads, V, X, labels, params, opts)


def test_forward_swept_in_bf16_then_the_family_runs_the_edge_pass_in_fp32(da):
    """one head of 32 features: the forward sweeps (bf16 rows, scores from the table), the row-wise destination side does not cover the
    shape; with the family forced for the backward its edge pass must not gather bf16 rows -- the per-layer flag is the family's alone"""
    assert not _dst_rowwise_covers(1, 32)
    ctx = _single(da, [24, 32, 8], [1, 2], 200, 1500, {"spmm_blk_nb": 8})
    try:
        ctx.gatmh_row_gather_bf16(1)
        ctx.set_option("gatmh_bf16_gather", 1)
        for l in range(2):
            ctx.apply_vertex(l, da.FORWARD)
            ctx.apply_edge(l + 1, da.FORWARD)
            ctx.aggregate(l + 1, da.FORWARD)
        assert counters(ctx) == (2, 0) and bf16_stats(ctx) == (0, 0, 0) and ctx.gatmh_row_gather_stats() == (0, 0, 0, 0)
        ctx.predict_gat(2)
        ctx.gatmh_row_gather(1)
        ctx.aggregate(2, da.BACKWARD)
        ctx.apply_vertex(1, da.BACKWARD)
        ctx.aggregate(1, da.BACKWARD)
        rows = ctx.gatmh_row_gather_stats()
        assert rows[0] == 0 and rows[1] >= 1 and rows[3] == 2, rows            # layer 0's destination side: an edge pass
        assert bf16_stats(ctx) == (0, 0, 0) and counters(ctx) == (2, 0)
        # the same layer once its forward ran the family's bf16 form: the edge pass follows it
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_edge(1, da.FORWARD)
        ctx.aggregate(1, da.FORWARD)
        ctx.aggregate(1, da.BACKWARD)
        assert bf16_stats(ctx) == (1, 1, 0), bf16_stats(ctx)
        # ... and a forward of another form clears the flag again
        ctx.gatmh_row_gather(0)
        ctx.aggregate(1, da.FORWARD)
        ctx.gatmh_row_gather(1)
        ctx.aggregate(1, da.BACKWARD)
        assert bf16_stats(ctx) == (1, 1, 0), bf16_stats(ctx)
    finally:
        ctx.close()


def test_refusals_that_stay(da):
    for gnn in (da.GCN, da.GAT):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        ctx.gatmh_row_gather_bf16(0)
        with pytest.raises(da.DoryError, match="DORY_GATMH"):
            ctx.gatmh_row_gather_bf16(1)
        ctx.close()
    ctx = da.Context(0)
    ctx.configure(da.GATMH, [24, 32, 8], 200)
    for bad in (-1, 2, 7):
        with pytest.raises(da.DoryError, match="0 or 1"):
            ctx.gatmh_row_gather_bf16(bad)
    ctx.close()
    # the switch on, but the call would take the blocked kernels (mode 0, one partition, a graph with a blocked layout, gatmh_sweep = 0)
    ctx = _single(da, [24, 32, 8], [4, 2], 200, 1500, {"spmm_blk_nb": 8})
    try:
        ctx.gatmh_row_gather_bf16(1)
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_edge(1, da.FORWARD)
        ctx.set_option("gatmh_sweep", 0)
        for v in (1, 2):
            ctx.set_option("gatmh_bf16_gather", v)
            with pytest.raises(da.DoryError, match="gatmh_sweep = 0"):
                ctx.aggregate(1, da.FORWARD)
        ctx.set_option("gatmh_bf16_gather", 0)
        ctx.aggregate(1, da.FORWARD)                     # (the blocked kernels, fp32)
        ctx.apply_vertex(1, da.FORWARD)
        ctx.apply_edge(2, da.FORWARD)
        ctx.aggregate(2, da.FORWARD)
        ctx.predict_gat(2)
        ctx.set_option("gatmh_bf16_gather", 2)
        with pytest.raises(da.DoryError, match="gatmh_sweep = 0"):
            ctx.aggregate(2, da.BACKWARD)
        # no layouts at all on one partition: the row-wise kernels of round 1, refused as before
        ctx.set_option("gatmh_blocked", 0)
        with pytest.raises(da.DoryError, match="gatmh_sweep = 0"):
            ctx.aggregate(2, da.BACKWARD)
        assert bf16_stats(ctx) == (0, 0, 0) and counters(ctx) == (0, 0) and ctx.gatmh_row_gather_stats() == (0, 0, 0, 0)
        ctx.set_option("gatmh_sweep", 1)
        ctx.set_option("gatmh_blocked", 1)
        ctx.set_option("gatmh_bf16_gather", 0)
        # inside a recording
        ctx.epoch_graph_begin()
        for on in (0, 1):
            with pytest.raises(da.DoryError, match="recorded"):
                ctx.gatmh_row_gather_bf16(on)
        ctx.epoch_graph_drop()
    finally:
        ctx.close()


# ---- 4. epoch graph -------------------------------------------------------------------------------------------------------------------
def test_replayed_epochs_are_bit_identical_to_eager(da):
    """single partition, mode 1, v = 2; layer 1 (one head of 6) takes the destination-side edge pass on bf16 rows"""
    dims, heads = [24, 64, 6], [4, 1]
    assert _dst_rowwise_covers(4, 64) and not _dst_rowwise_covers(1, 6)
    states = []
    for graph in (0, 1):
        ctx = _single(da, dims, heads, 300, 4000, {})
        ctx.gatmh_row_gather(1)
        ctx.gatmh_row_gather_bf16(1)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.adam_config(0.01)
        ctx.set_option("epoch_graph", graph)
        eng = da.NativeEngine(ctx)
        eng.run(3)
        eng.run(2)
        if graph:                               # one eager epoch and one recording: replays do not count
            assert ctx.get_option("epoch_graph_recorded") == 1
            assert bf16_stats(ctx) == (4, 2, 4), bf16_stats(ctx)
        else:
            assert bf16_stats(ctx) == (10, 5, 10), bf16_stats(ctx)
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


def test_shadow_rows_cannot_grow_inside_a_recording(da):
    ctx = _single(da, [24, 64, 6], [4, 1], 300, 4000, {})
    try:
        ctx.gatmh_row_gather(1)
        ctx.gatmh_row_gather_bf16(1)
        ctx.adam_config(0.01)
        eng = da.NativeEngine(ctx)
        eng.run(1)                                           # an eager fp32 epoch: every other lazily sized buffer exists
        assert bf16_stats(ctx) == (0, 0, 0)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.epoch_graph_begin()
        ctx.apply_vertex(0, da.FORWARD)
        ctx.apply_edge(1, da.FORWARD)
        with pytest.raises(da.DoryError, match="gatmh_bf16_gather would have to grow"):
            ctx.aggregate(1, da.FORWARD)
        ctx.epoch_graph_drop()
        assert bf16_stats(ctx) == (0, 0, 0)
        eng.run(1)                                           # eager, with the option: the rows exist now
        assert bf16_stats(ctx) == (2, 1, 2)
        ctx.set_option("epoch_graph", 1)
        eng.run(3)
        assert ctx.get_option("epoch_graph_recorded") == 1
        assert bf16_stats(ctx) == (4, 2, 4)
        eng.close()
    finally:
        ctx.close()


# ---- 5. the bf16 wire -----------------------------------------------------------------------------------------------------------------
def _local_run(da, wire, merged):
    """two ranks over dory_comm_init_local, two epochs, whole sweeps, mode 1, v = 2; 8 x 16 then one head of 6: the scores come from the
    gathered row on both layers (no kernel of the family reads fg_el)"""
    from local_ranks import run_local
    dims, heads = DIMS8, HEADS8
    s, d, parts, rng = _hub_graph(2)
    parts = parts.astype(np.int32)
    V = len(parts)
    X, labels, params = _inputs(rng, V, dims, heads)
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "h", X[g["localToGlobal"]])
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.gatmh_row_gather(1)
        ctx.gatmh_row_gather_bf16(1)
        ctx.gatmh_bwd_merged_exchange(merged)
        ctx.halo_bf16_rows(wire)
        ctx.gatmh_halo_bf16(wire)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = (bf16_stats(ctx), ctx.gatmh_halo_bf16_stats(), ctx.gatmh_bwd_merged_exchange_stats())
            close()
        ctx.close = closing
    pobjs = [da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, 2) for r in range(2)]
    dl = [(l, nm) for l in range(2) for nm in ("z", "el", "er", "o", "op", "m", "den", "dpos", "do", "t", "del", "der", "st", "dz")]
    dl += [(1, "logits"), (1, "grad"), (1, "h")]
    out = run_local(da, pobjs, parts, dims, da.GATMH, 2, setup, {"gatmh_bwd_phase": 0, "gatmh_bf16_gather": 2}, downloads=dl,
                    pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r"))
    return out, kept


def test_bf16_wire_off_against_on_and_merged_exchange(da):
    """dory_halo_bf16_rows + dory_gatmh_halo_bf16 now reach the family's ranks: z ships bf16 forward, do backward.  Rounding is
    idempotent and every gather of fg_z / bg_do reads the shadow rows, so every local tensor, weight and gradient is the same bits"""
    off, k_off = _local_run(da, 0, 0)
    runs = [_local_run(da, 1, 0), _local_run(da, 1, 1)]
    for r in range(2):
        assert k_off[r][0] == (4, 2, 4) and k_off[r][1][:3] == (0, 0, 0), (r, k_off[r])
    for on, k_on in runs:
        for r in range(2):
            assert len(off["tensors"][r]) >= 30 and off["tensors"][r].keys() == on["tensors"][r].keys()
            for k in off["tensors"][r]:
                assert same_bits(off["tensors"][r][k], on["tensors"][r][k]), (r, k)
            for l in range(2):
                for nm in ("w", "a_l", "a_r"):
                    assert same_bits(off["weights"][r][l][nm], on["weights"][r][l][nm]), (r, l, nm)
                    assert same_bits(off["wgrads"][r][l][nm], on["wgrads"][r][l][nm]), (r, l, nm)
            stats, wire, merged = k_on[r]
            assert stats == (4, 2, 4), (r, stats)
            assert wire[0] > 0 and wire[1] > 0 and wire[2] > 0, (r, wire)          # bf16 rows were shipped, forward and backward
    assert runs[0][1][0][2][0] == 0 and runs[1][1][0][2][0] == 4, (runs[0][1][0][2], runs[1][1][0][2])       # merged exchanges: off, on


# ---- 6. learning ----------------------------------------------------------------------------------------------------------------------
def test_planted_communities_are_learned_with_bf16_rows(da):
    """the model, task, epochs and criterion of tests/test_gpu_gatmh_bf16_gather.py::test_planted_communities_are_learned_with_bf16_rows
    (4 heads x 8, then two heads of 8 logits), on the row-gather family with v = 2"""
    from test_gpu_learning import _task
    s, d, X, y, C = _task()
    V, F = X.shape
    part = da.Partition.build(s, d, np.zeros(V, np.int32), 0, 1)
    ctx = da.Context(0)
    ctx.configure(da.GATMH, [F, 32, 8], V)
    ctx.gatmh_heads([4, 2])
    part.upload(ctx)
    ctx.preallocate()
    ctx.upload(0, "h", X)
    ctx.labels_upload(y)
    ctx.weights_init_xavier()
    rng = np.random.default_rng(1)
    for l, zw in ((0, 32), (1, 16)):
        ctx.weight_set(l, "a_l", (rng.standard_normal(zw) * 0.1).astype(np.float32))
        ctx.weight_set(l, "a_r", (rng.standard_normal(zw) * 0.1).astype(np.float32))
    ctx.adam_config(0.01)
    ctx.gatmh_row_gather(1)
    ctx.gatmh_row_gather_bf16(1)
    ctx.set_option("gatmh_bf16_gather", 2)
    eng = da.NativeEngine(ctx)
    acc = []
    for _ in range(12):
        eng.run(5)
        logits = ctx.download(1, "logits")
        lo, hi = int(V * 0.66), int(V * 0.66) + int(V * 0.1)
        acc.append(float((logits[lo:hi].argmax(1) == y[lo:hi]).mean()))
    st = bf16_stats(ctx)
    eng.close()
    ctx.close()
    assert st[0] == 120 and st[2] == 120, st
    print(f"\ngatmh row gather, bf16 rows: validation accuracy {acc[0]:.3f} -> {acc[-1]:.3f}")
    assert acc[-1] > 0.85 and acc[-1] > acc[0], acc
