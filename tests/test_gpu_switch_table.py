"""The ten feature switches dory_<name>(ctx, int) on real contexts: one context per model walked through its states -- created,
configured, preallocated as rank 0 of 2, recording an epoch graph as a single partition -- and in each state every setter called with
0, 1 and 2.  Return code and dory_last_error text must be the literals of tests/test_switch_table.py for that state (imported, not
restated); after each accepted call every _stats entry point still reports zeros and twin_bytes what the rule of dory_halo_bf16_ghosts
gives.  Then the two hooks with a consequence a caller can see: dory_halo_bf16_ghosts(0) turns dory_gatmh_bf16_ghosts off and frees
its twins, and a refused dory_gatmh_bwd_merged_exchange(1) leaves the switch as it was."""
import threading

import numpy as np
import pytest

import halo_exact_ref as hx
from test_switch_table import ERR_ARG, OK, PARENT, SWITCHES, State, expected

pytestmark = pytest.mark.gpu
V, E = 60, 400
MODELS = {"GCN": ([4, 41, 2], None), "GAT": ([4, 16, 2], None), "GATMH": ([16, 32, 8], [4, 1])}
STATS_DICTS = ("halo_bf16_ghosts", "gatmh_bf16_ghosts")   # the two whose Context method returns a dict


@pytest.fixture(scope="module")
def da():
    import torch  # noqa: F401  (one HIP runtime in the process)
    import dorylus_amd
    return dorylus_amd


def _graph(seed=60):
    rng = np.random.default_rng(seed)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    src, dst = np.concatenate([s, d]).astype(np.uint32), np.concatenate([d, s]).astype(np.uint32)
    return src, dst, (rng.permutation(V) % 2).astype(np.int32)


def _configure(da, ctx, model, node_id, num_nodes):
    dims, heads = MODELS[model]
    ctx.configure(getattr(da, model), dims, V, node_id, num_nodes)
    if heads:
        ctx.gatmh_heads(heads)


def _twin_bytes(model, gi, go):
    """the bytes of the twins dory_halo_bf16_ghosts allocates (with dory_gatmh_bf16_ghosts on top for the multi-head GAT): rows x ld x 2
    for every ghost tensor an exchange can fill -- as tests/test_gpu_gatmh_bf16_ghosts.py::test_refusals_and_the_switch_underneath"""
    dims, heads = MODELS[model]
    ld = hx.pad_ld
    if model == "GCN":      # fg@1 and bg@0 (41 floats); the transform-first pair of layer 1 (41 > 2): fgxw@1, bgg@1 (2 floats); never fg@0
        return 2 * (gi * (ld(41) + ld(2)) + go * (ld(41) + ld(2)))
    widths = (16, 2) if model == "GAT" else (32, 8 * 1)     # fg_z / bg_d, fg_z / bg_do of both layers
    return 2 * sum((gi + go) * ld(w) for w in widths)


class Walk:
    """a context, the state the literals are asked about, and the switches it has accepted so far"""

    def __init__(self, da, model):
        self.da, self.model, self.ctx = da, model, da.Context(0)
        self.gnn = getattr(da, model)
        self.configured = self.prealloc = self.recording = False
        self.on = dict.fromkeys(SWITCHES, 0)
        self.ghosts = (0, 0)

    def twin_bytes(self):
        kept = self.on["halo_bf16_ghosts"] and (self.model != "GATMH" or self.on["gatmh_bf16_ghosts"])
        return _twin_bytes(self.model, *self.ghosts) if kept else 0

    def check_stats(self, what):
        for name in SWITCHES:
            got = getattr(self.ctx, name + "_stats")()
            vals = dict(got) if name in STATS_DICTS else dict(enumerate(got))
            assert vals.pop("twin_bytes", 0) == (self.twin_bytes() if name == "halo_bf16_ghosts" else 0), (what, name, got)
            assert set(vals.values()) == {0}, (what, name, got)

    def call_all(self, what):
        lib, h = self.ctx.lib, self.ctx.h
        accepted = 0
        for value in (0, 1, 2):                 # value by value: every switch off, then on (the parent before its child), then refused
            for name in SWITCHES:
                s = State(value, self.gnn, self.configured, self.prealloc, self.recording, bool(self.on[PARENT[name]]) if name in PARENT else False)
                rc = getattr(lib, "dory_" + name)(h, value)
                got = (rc, lib.dory_last_error(h).decode() if rc else "")
                assert got == expected(name, s), (what, name, s)
                if rc == OK:
                    accepted += 1
                    self.on[name] = value
                    if name == "halo_bf16_ghosts" and not value:
                        self.on["gatmh_bf16_ghosts"] = 0
                    self.check_stats((what, name, value))
        return accepted


@pytest.mark.parametrize("model", list(MODELS))
def test_every_setter_in_every_state_answers_the_literals(da, model):
    src, dst, parts = _graph()
    w = Walk(da, model)
    try:
        assert w.call_all("created") == 2                                       # "off" of the row-gather pair is legal on any context
        _configure(da, w.ctx, model, 0, 2)
        w.configured = True
        w.call_all("configured")
        part = da.Partition.build(src, dst, parts, 0, 2)
        part.upload(w.ctx, parts)
        w.ctx.preallocate()
        w.prealloc = True
        g = part.view()
        w.ghosts = (int(g["srcGhostCnt"]), int(g["dstGhostCnt"]))
        assert min(w.ghosts) > 0
        w.call_all("preallocated")
        assert w.on["halo_bf16_ghosts"] == 1 and w.on["gatmh_bf16_ghosts"] == (model == "GATMH") and w.twin_bytes() > 0
    finally:
        w.ctx.close()
    # recording: a single partition (an epoch graph records no other)
    w = Walk(da, model)
    try:
        _configure(da, w.ctx, model, 0, 1)
        da.Partition.build(src, dst, np.zeros(V, np.int32), 0, 1).upload(w.ctx)
        w.ctx.preallocate()
        w.configured = w.prealloc = True
        w.ctx.epoch_graph_begin()
        w.recording = True
        assert w.call_all("recording") == 2                                     # dory_halo_fused_pack alone takes 0 and 1 inside a recording
        w.ctx.epoch_graph_drop()
    finally:
        w.ctx.close()


def test_halo_bf16_ghosts_off_turns_gatmh_bf16_ghosts_off_and_frees_its_twins(da):
    src, dst, parts = _graph()
    ctx = da.Context(0)
    try:
        _configure(da, ctx, "GATMH", 0, 2)
        part = da.Partition.build(src, dst, parts, 0, 2)
        part.upload(ctx, parts)
        ctx.preallocate()
        g = part.view()
        want = _twin_bytes("GATMH", int(g["srcGhostCnt"]), int(g["dstGhostCnt"]))
        ctx.halo_bf16_ghosts(1)
        ctx.gatmh_bf16_ghosts(1)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == want > 0 and ctx.halo_bf16_ghost_peek(0, "fg_z")[0]
        ctx.halo_bf16_ghosts(0)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0 and ctx.halo_bf16_ghost_peek(0, "fg_z")[0] is None
        # the child went off with it: the parent alone brings no twin back, and the child is refused until the parent is on again
        assert ctx.lib.dory_gatmh_bf16_ghosts(ctx.h, 0) == ERR_ARG
        assert ctx.lib.dory_last_error(ctx.h).decode() == expected("gatmh_bf16_ghosts", State(0, da.GATMH, True, True, False, False))[1]
        ctx.halo_bf16_ghosts(1)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == 0
        ctx.gatmh_bf16_ghosts(1)
        assert ctx.halo_bf16_ghosts_stats()["twin_bytes"] == want
    finally:
        ctx.close()


def test_a_refused_merged_exchange_leaves_the_switch_unchanged(da):
    """Two in-process ranks whose plans sized the buffers with the switch off; the hidden layer's merged row (96 floats of do + 4 of
    st) is wider than any padded row of the model (96), so dory_gatmh_bwd_merged_exchange(1) after dory_comm_init_local is refused:
    the peers hold the buffers' addresses.  Were the switch stored all the same, the epoch that follows would take the merged exchange and fail on
    those buffers; it runs, and counts no merged exchange and no split fallback (which only a switch that is on counts)."""
    dims, heads = [12, 80, 6], [1, 1]       # (a shape tests/test_gpu_gatmh_row_gather.py runs on two ranks, mode 1)
    src, dst, parts = _graph()
    rng = np.random.default_rng(3)
    ctxs = []
    try:
        for r in range(2):
            part = da.Partition.build(src, dst, parts, r, 2)
            ctx = da.Context(0)
            ctxs.append(ctx)
            ctx.configure(da.GATMH, dims, V, r, 2)
            ctx.gatmh_heads(heads)
            ctx.set_option("local_timeout_ms", 5000)
            part.upload(ctx, parts)
            ctx.preallocate()
            n = int(part.view()["localVtxCnt"])
            ctx.upload(0, "h", rng.uniform(-1, 1, (n, dims[0])).astype(np.float32))
            ctx.labels_upload(rng.integers(0, dims[-1], n).astype(np.uint32))
            ctx.weights_init_xavier()
            ctx.adam_config(0.01)
            ctx.gatmh_row_gather(1)
        for c in ctxs:
            c.sync()
        da.Context.comm_init_local(ctxs)
        for c in ctxs:
            assert c.lib.dory_gatmh_bwd_merged_exchange(c.h, 1) == ERR_ARG
            assert c.lib.dory_last_error(c.h).decode() == ("gatmh_bwd_merged_exchange: the exchange buffers are too small for merged rows and the "
                                                           "in-process peers hold their addresses: call it before dory_comm_init_local")
        engs = [da.NativeEngine(c) for c in ctxs]
        errors = [None, None]

        def drive(r):
            try:
                engs[r].run(1)
                ctxs[r].sync()
            except Exception as e:
                errors[r] = e
        th = [threading.Thread(target=drive, args=(r,)) for r in range(2)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert errors == [None, None], errors
        for c in ctxs:
            assert c.gatmh_bwd_merged_exchange_stats() == (0, 0, 0, 0)
        for e in engs:
            e.close()
        for c in ctxs:
            c.gatmh_bwd_merged_exchange(0)      # "off" needs no buffers: accepted
    finally:
        for c in ctxs:
            c.close()
