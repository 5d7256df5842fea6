"""dory_gatmh_row_gather_bf16_wide (include/dorylus_hip.h): the wide (16-byte) bf16 form of the multi-head GAT's row-gather kernels
(csrc/gat_mh_rows.hip, gatmh_rows8_*_kernel).  A wide lane keeps two float4s of a row and stands for two lanes of the narrow bf16 form;
per column the sums are the same fmaf chains, per head the values the same scalar chains, and a dot product is the narrow lanes' two
chains added in the lane and reduced by the same butterfly over half the lanes (tests/test_gatmh_row_gather_bf16_wide_reference.py).  So
the contract is BIT EQUALITY with the narrow bf16 form in every tensor a pass writes.

The scheme of tests/test_gpu_gatmh_row_gather_bf16.py, stage by stage through the C-ABI, on every rank of a run:
  context A: gatmh_row_gather(1), gatmh_row_gather_bf16(1), gatmh_bf16_gather = 2, gatmh_row_gather_bf16_wide(1);   context B: the same, wide off.
Asserted bit for bit after every stage: o, op, m, den, dpos, the next h / logits, t, der, st, del, dz and the gradients of a_l / a_r / w;
A's wide counters moved by exactly the passes the shape rule (dory_gatmh_row_gather_bf16_wide_form) predicts per layer and
narrow_while_on for the others, B's did not move, and the family's bf16 counters are equal in A and B."""
import numpy as np
import pytest

from test_gpu_gatmh_bf16_gather import same_bits
from test_gpu_gatmh_row_gather import _hub_graph, _layer_shapes, _pad_ld
from test_gpu_gatmh_row_gather_bf16 import BWD_NAMES, FWD_NAMES, Ranks, _inputs, bf16_stats

pytestmark = pytest.mark.gpu

# one shape per wide instantiation -- (lanes per row, scores from the gathered row) of layer 0 / layer 1:
WIDE = [([24, 64, 41], [8, 1]),       # 8 x 8 (a head is one lane: no lane step) and 1 x 41 on 64 floats: 8 lanes
        ([24, 64, 6], [4, 1]),        # 4 x 16 on 8 lanes; layer 1 (1 x 6, ld = 32) stays narrow
        ([24, 128, 6], [8, 1]),       # 8 x 16: 16 lanes
        ([24, 128, 6], [2, 1]),       # 2 x 64: eight lanes a head
        ([24, 256, 9], [32, 1]),      # 32 x 8: 32 lanes
        ([24, 256, 6], [4, 1]),       # 4 x 64
        ([12, 100, 6], [1, 1]),       # one head of 100 on 128 floats: the head is the 16-lane group, dead lanes at its end
        ([12, 256, 6], [1, 1]),       # one head on 32 lanes: the widest reduction
        ([24, 96, 6], [3, 1]),        # 96 floats: 16 lanes, scores gathered
        ([24, 160, 5], [5, 1]),       # 160 floats: 32 lanes, scores gathered
        ([12, 200, 6], [1, 1])]       # one head of 200 on 224 floats: 32 lanes (28 live), scores gathered
NARROW = [([24, 32, 8], [4, 2]), ([24, 64, 6], [32, 1]), ([16, 32, 5], [32, 1])]       # ld = 32, D = 2, D = 1: only the fallback counter moves
DIMS8, HEADS8 = [24, 128, 6], [8, 1]
PARTITIONED = [(DIMS8, HEADS8), ([24, 64, 41], [8, 1]), ([24, 96, 6], [3, 1])]
WIDE_ZERO = {"fwd": 0, "dst_edge_pass": 0, "src": 0, "narrow_while_on": 0}


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def wide_layers(da, dims, heads):
    """per layer: does a bf16 pass of the family take the wide form (the rule, asked of the library without a context)"""
    return [da.gatmh_row_gather_bf16_wide_form(K, zw // K, _pad_ld(zw)) is not None for K, zw in _layer_shapes(dims, heads)]


class SwitchedDa:
    """the package as the helpers of the other test files see it, with contexts that have the family's other switches set from birth"""

    def __init__(self, da, chunk=0, overlap=0):
        self._da, self.chunk, self.overlap = da, chunk, overlap

    def __getattr__(self, k):
        return getattr(self._da, k)

    def Context(self, device=0):
        ctx = self._da.Context(device)
        ctx.gatmh_row_gather_hub_split(self.chunk)
        ctx.gatmh_row_gather_overlap(self.overlap)
        return ctx


class WideRanks(Ranks):
    """Ranks with BOTH sides on the family's bf16 form (option gatmh_bf16_gather = v) and the wide switch on in A alone: nothing is
    rounded on the host, the stages' bits are compared as they are.  v = 0 with bf16_switch = False: the fp32 family on both sides."""

    def __init__(self, da, gs, parts, X, labels, params, dims, heads, v, bf16_switch=True, **kw):
        super().__init__(da, gs, parts, X, labels, params, dims, heads, v, **kw)
        for r in range(self.P):
            for c in (self.A[r], self.B[r]):
                c.gatmh_row_gather_bf16(1 if bf16_switch else 0)
                c.set_option("gatmh_bf16_gather", v)
            self.A[r].gatmh_row_gather_bf16_wide(1)
        self.wide = wide_layers(da, dims, heads)
        self.bexp = [0, 0, 0]                                 # the family's bf16 passes (every live rank alike): fwd, dst edge pass, src
        self.wexp = dict(WIDE_ZERO)

    def round_in_b(self, l, local, ghost):
        return []

    def check_counters(self, where):
        kind, l = where
        i = {"forward": 0, "phase 1": 1, "phase 2": 2}[kind]
        ran_bf16 = self.v >= (2 if i == 2 else 1) and (i != 1 or self.edge_pass(l))
        if ran_bf16:
            self.bexp[i] += 1
            self.wexp[("fwd", "dst_edge_pass", "src")[i] if self.wide[l] else "narrow_while_on"] += 1
        for r in self.live:
            assert bf16_stats(self.A[r]) == tuple(self.bexp) == bf16_stats(self.B[r]), (where, r, bf16_stats(self.A[r]), bf16_stats(self.B[r]), self.bexp)
            assert self.A[r].gatmh_row_gather_bf16_wide_stats() == self.wexp, (where, r, self.A[r].gatmh_row_gather_bf16_wide_stats(), self.wexp)
            assert self.B[r].gatmh_row_gather_bf16_wide_stats() == WIDE_ZERO, (where, r)
            assert self.A[r].gatmh_row_gather_stats() == self.B[r].gatmh_row_gather_stats(), (where, r)

    def state(self):
        """every tensor an epoch leaves, per rank of side A"""
        out = []
        for r in self.live:
            st = {}
            for l in range(2):
                for nm in FWD_NAMES + BWD_NAMES:
                    st[(l, nm)] = self.A[r].download(l, nm)
                for nm in ("a_l", "a_r", "w"):
                    st[(l, "d" + nm)] = self.A[r].weight_grad_get(l, nm)
            st["logits"] = self.A[r].download(1, "logits")
            out.append(st)
        return out


def _ranks(da, P, dims, heads, v=2, blocks=False, **kw):
    """the hub graph of tests/test_gpu_gatmh_row_gather.py (scattered ownership: every row a boundary row), or -- blocks -- the block
    graph of tests/test_gpu_gatmh_row_gather_overlap.py (interior and boundary rows on both adjacencies, an interior hub on rank 0)"""
    import partition_oracle as po
    if blocks:
        from test_gpu_gatmh_row_gather_overlap import _case
        s, d, parts, rng, gs, _ = _case(da, P)
    else:
        s, d, parts, rng = _hub_graph(P)
        gs = [po.preprocess(s, d, parts if P > 1 else np.zeros(len(parts), np.int64), r, P) for r in range(P)]
    V = len(parts)
    if P > 1:
        assert all(int(g["srcGhostCnt"]) and int(g["dstGhostCnt"]) for g in gs)      # ghost rows on both adjacencies of every rank
    X, labels, params = _inputs(rng, V, dims, heads)
    return WideRanks(da, gs, parts, X, labels, params, dims, heads, v, **kw)


def _run(da, P, dims, heads, **kw):
    """one epoch, A against B after every stage; returns A's final wide counters (every live rank's are alike: asserted by the stages)"""
    R = _ranks(da, P, dims, heads, **kw)
    try:
        R.epoch()
        edge = [R.edge_pass(l) for l in range(2)]
        st = R.A[R.live[0]].gatmh_row_gather_bf16_wide_stats()
        want = {"fwd": sum(R.wide), "dst_edge_pass": sum(w and e for w, e in zip(R.wide, edge)), "src": sum(R.wide),
                "narrow_while_on": sum((not w) * (2 + e) for w, e in zip(R.wide, edge))}
        assert st == want, (st, want)
        return st, R
    finally:
        R.close()


# ---- 1. A against B over every wide instantiation, and the shapes that stay narrow --------------------------------------------------------
@pytest.mark.parametrize("dims,heads", WIDE)
def test_wide_passes_equal_narrow_passes_bit_for_bit(da, dims, heads):
    st, R = _run(da, 1, dims, heads)
    assert R.wide[0] and st["fwd"] >= 1 and st["src"] >= 1, st


@pytest.mark.parametrize("dims,heads", NARROW)
def test_shapes_without_a_wide_form_run_narrow_and_are_counted(da, dims, heads):
    st, R = _run(da, 1, dims, heads)
    assert R.wide == [False, False]
    assert (st["fwd"], st["dst_edge_pass"], st["src"]) == (0, 0, 0) and st["narrow_while_on"] >= 4, st


@pytest.mark.parametrize("P", [2, 3])
@pytest.mark.parametrize("dims,heads", PARTITIONED)
def test_partitioned_with_ghost_rows_on_both_adjacencies(da, dims, heads, P):
    _run(da, P, dims, heads)


# ---- 2. with the family's other switches, 8 x 16 on two ranks ----------------------------------------------------------------------------
def _with_switches(da, chunk, overlap, opts=None, blocks=False):
    R = _ranks(SwitchedDa(da, chunk=chunk, overlap=overlap), 2, DIMS8, HEADS8, opts=opts, blocks=blocks)
    try:
        R.epoch()
        out = []
        for r in R.live:
            a, b = R.A[r], R.B[r]
            assert a.gatmh_row_gather_hub_split_stats() == b.gatmh_row_gather_hub_split_stats(), r
            assert a.gatmh_row_gather_overlap_stats() == b.gatmh_row_gather_overlap_stats(), r
            out.append((a.gatmh_row_gather_hub_split_stats(), a.gatmh_row_gather_overlap_stats(), a.gatmh_row_gather_bf16_wide_stats()))
        return out
    finally:
        R.close()


def test_hub_rows_in_chunks_of_64(da):
    """the *_hub bodies leave their chunk states where the narrow lanes leave them: the narrow merge kernels fold them"""
    out = _with_switches(da, 64, 0, opts={"gatmh_sweep": 0})
    total = {k: sum(hub[k] for hub, _, _ in out) for k in out[0][0]}      # (the hub destination and the hub source: on whichever ranks)
    assert total["in_chunks"] >= 4 and total["out_chunks"] >= 4 and total["fwd"] >= 2 and total["dst_edge_pass"] >= 2 and total["src"] >= 2, total
    for hub, ovl, wide in out:
        assert wide["fwd"] == 1 and wide["dst_edge_pass"] == 1 and wide["src"] == 1, wide           # layer 0 (8 x 16); layer 1 is ld = 32


@pytest.mark.parametrize("chunk", [0, 64])
def test_interior_rows_beside_the_exchange(da, chunk):
    """overlap on: the *_list bodies, and with chunk 64 the *_list_hub bodies"""
    out = _with_switches(da, chunk, 1, blocks=True)
    for hub, ovl, wide in out:
        assert ovl["fwd_split"] == 2 and ovl["src_split"] == 2, ovl
        assert wide["fwd"] == 1 and wide["src"] == 1, wide
    assert (out[0][0]["in_chunks"] > 0 and out[0][0]["out_chunks"] > 0) == (chunk != 0), out[0][0]      # (rank 0 owns the hubs)


def test_edge_pass_on_every_layer(da):
    st, R = _run(da, 2, DIMS8, HEADS8, opts={"gatmh_sweep": 0})
    assert st["dst_edge_pass"] == 1 and st["narrow_while_on"] == 3, st


def test_bf16_wire_and_ghost_twins(da):
    """dory_halo_bf16_rows + dory_gatmh_halo_bf16 + dory_gatmh_bf16_ghosts (tests/test_gpu_gatmh_bf16_ghosts.py::Stages: the rows delivered
    through dory_halo_unpack / dory_gatmh_bwd_unpack): the wide gathers read the twins.  Stages asserts twins on = twins off at every
    stage; run with the wide switch on and off in all its contexts, the two runs leave the same bits"""
    from test_gpu_gatmh_bf16_ghosts import Stages

    class WideDa(SwitchedDa):
        def __init__(self, da, on):
            super().__init__(da)
            self.on = on

        def Context(self, device=0):
            ctx = super().Context(device)
            ctx.gatmh_row_gather_bf16_wide(self.on)
            return ctx

    states = []
    for on in (1, 0):
        S = Stages(WideDa(da, on), DIMS8, HEADS8, 2)
        try:
            S.epoch()
            st = {}
            for r in range(2):
                for l in range(2):
                    for nm in FWD_NAMES + BWD_NAMES:
                        st[(r, l, nm)] = S.A[r].download(l, nm)
                    for nm in ("a_l", "a_r", "w"):
                        st[(r, l, "d" + nm)] = S.A[r].weight_grad_get(l, nm)
                st[(r, "logits")] = S.A[r].download(1, "logits")
                wide = S.A[r].gatmh_row_gather_bf16_wide_stats()
                assert S.A[r].gatmh_bf16_ghosts_stats()["twin_reads_rows"] > 0
                assert wide == S.B[r].gatmh_row_gather_bf16_wide_stats()
                assert wide == ({"fwd": 1, "dst_edge_pass": 0, "src": 1, "narrow_while_on": 3} if on else WIDE_ZERO), (on, r, wide)
            states.append(st)
        finally:
            S.close()
    assert states[0].keys() == states[1].keys() and len(states[0]) == 54
    for k in states[0]:
        assert same_bits(states[0][k], states[1][k]), k


# ---- 3. the setter ----------------------------------------------------------------------------------------------------------------------------
def test_refusals_and_values(da):
    for gnn in (da.GCN, da.GAT):
        ctx = da.Context(0)
        ctx.configure(gnn, [16, 8, 3], 100)
        ctx.gatmh_row_gather_bf16_wide(0)
        with pytest.raises(da.DoryError, match="DORY_GATMH"):
            ctx.gatmh_row_gather_bf16_wide(1)
        assert ctx.gatmh_row_gather_bf16_wide_stats() == WIDE_ZERO
        ctx.close()
    from test_gpu_gatmh_row_gather_bf16 import _single
    ctx = _single(da, [24, 64, 6], [4, 1], 200, 1500, {})
    try:
        for bad in (2, -1):
            with pytest.raises(da.DoryError, match="neither 0 nor 1"):
                ctx.gatmh_row_gather_bf16_wide(bad)
        ctx.gatmh_row_gather_bf16_wide(1)
        ctx.gatmh_row_gather_bf16_wide(0)
        ctx.epoch_graph_begin()
        for on in (0, 1):
            with pytest.raises(da.DoryError, match="recorded"):
                ctx.gatmh_row_gather_bf16_wide(on)
        ctx.epoch_graph_drop()
        ctx.gatmh_row_gather_bf16_wide(1)
        assert ctx.gatmh_row_gather_bf16_wide_stats() == WIDE_ZERO
    finally:
        ctx.close()


def test_inert_while_the_bf16_switch_is_off(da):
    """wide on, dory_gatmh_row_gather_bf16 off, gatmh_bf16_gather = 0: the fp32 family runs in A as in B, no counter moves"""
    R = _ranks(da, 2, DIMS8, HEADS8, v=0, bf16_switch=False)
    try:
        R.epoch()
        for r in R.live:
            assert R.A[r].gatmh_row_gather_bf16_wide_stats() == WIDE_ZERO and bf16_stats(R.A[r]) == (0, 0, 0)
            assert R.A[r].gatmh_row_gather_stats()[0] == 2 and R.A[r].gatmh_row_gather_stats()[3] == 2
    finally:
        R.close()


# ---- 4. repeatability ----------------------------------------------------------------------------------------------------------------------
def test_a_wide_epoch_run_twice_gives_the_same_bits(da):
    R = _ranks(SwitchedDa(da, chunk=64), 2, DIMS8, HEADS8)
    try:
        R.epoch()
        first = R.state()
        R.epoch()
        second = R.state()
        for a, b in zip(first, second):
            for k in a:
                assert same_bits(a[k], b[k]), k
    finally:
        R.close()
