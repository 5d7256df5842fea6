"""The reference's scatter messages on the device (include/dorylus_hip.h: dory_halo_wire_ids, dory_scatter_msgs_layout / _pack /
_deliver / _finish, dory_comm_set_scatter_transport) against the numpy restatement of the reference's sender and receiver loops
(tests/scatter_msg_ref.py).

  1. pack: every rank of the golden partitions, forward and backward, rows of 1 .. 602 floats, four message sizes -- every message
     byte for byte what the restatement sends, zeros between the messages, nothing behind the buffer, no NaN out of the source's
     poisoned padding; the GAT prototype's tensors and the multi-head GAT's "do" / "st" by name;
  2. deliver: each rank's messages into their receivers -- ghost rows bit-equal to the owners' rows, the raw ld-wide rows bit-equal
     to what the dense split unpack leaves, from a ghost tensor that held NaN everywhere; records shuffled, messages re-cut,
     senders interleaved, one message per call and all in one, option halo_direct_recv 0 and 1;
  3. errors: unknown id, duplicate, missing record (counted on the device, DORY_ERR_COMM at the finish, the other rows written, the
     next round clean); featDim mismatch, truncated message, foreign or malformed receiver, layer out of range (DORY_ERR_ARG, the
     text names the field, nothing written);
  4. the transport: two and three processes on one device, gloo carries the messages as bytes; GCN 64-41-7 for three epochs and one
     GAT-prototype epoch give, tensor by tensor and weight by weight, the bits of the same run over dory_comm_set_host_transport
     (once with halo_exact_rows on the dense side, once with halo_direct_recv on both), with halo_overlap on and off."""
import ctypes as C
import glob
import os
import socket
import struct
import sys
import traceback

import numpy as np
import pytest

import scatter_msg_ref as sm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = ("parts_toy60_p2", "parts_toy40_p3_empty", "parts_toy60_p4_hash", "parts_toy97_p8_und", "parts_hub3000_p2")
WIDTHS = (1, 3, 4, 41, 48, 128, 130, 602)
# one GCN context per rank covers every width: the forward exchange of layer l ships h@(l-1) into fg@l, the backward one grad@l
# into bg@(l-1), both dims[l] floats wide
DIMS = [4] + list(WIDTHS) + [2]
ERR_ARG, ERR_COMM = -1, -4
GUARD = 256


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _hip():
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    return hip


def _raw_rows(ctx, layer, name):
    """the raw ld-wide rows of a device tensor, through its dory_tensor_info pointer"""
    rows, cols, ld, p = ctx.info(layer, name)
    out = np.empty((rows, ld), np.float32)
    if rows:
        ctx.sync()
        assert _hip().hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) == 0
    return out


def _fill_nan(ctx, layer, name):
    """NaN into every float of a device tensor, padding included"""
    rows, cols, ld, p = ctx.info(layer, name)
    if rows:
        a = np.full((rows, ld), np.nan, np.float32)
        ctx.sync()
        assert _hip().hipMemcpy(C.c_void_p(p), a.ctypes.data_as(C.c_void_p), a.nbytes, 1) == 0


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _golden(da, name):
    d = os.path.join(ROOT, "tests", "golden", name)
    bins = sorted(glob.glob(os.path.join(d, "graph.*.bin")), key=lambda p: int(p.split(".")[-2]))
    parts = np.loadtxt(os.path.join(d, "graph.bsnap.parts"), dtype=np.int32, ndmin=1)
    return [da.Partition.load(b) for b in bins], parts


def _src(layer, direction):
    """(layer, name) of the tensor the exchange (layer, direction) of a GCN context ships, of its ghost tensor, and the layer its messages name"""
    return ((layer - 1, "h"), (layer, "fg"), layer) if direction == 0 else ((layer, "grad"), (layer - 1, "bg"), layer - 1)


class Ranks:
    """every rank of a golden case as a GCN context of DIMS; the rows every exchange ships are slices of one table per
    (layer, direction) over the global vertices, so that every rank's messages and ghost rows are known on the host"""

    def __init__(self, da, case, direct):
        from helpers import _poison_padding
        self.pobjs, self.parts = _golden(da, case)
        self.views = [p.view() for p in self.pobjs]
        self.P, V = len(self.pobjs), len(self.parts)
        rng = np.random.default_rng(len(case))
        self.tab = {(l, d): rng.standard_normal((V, DIMS[l])).astype(np.float32) for l in range(1, len(WIDTHS) + 1) for d in (0, 1)}
        self.ctxs = []
        for r, part in enumerate(self.pobjs):
            ctx = da.Context(0)
            ctx.configure(da.GCN, DIMS, V, r, self.P)
            ctx.set_option("halo_direct_recv", direct)
            part.upload(ctx, self.parts)              # adjacency, both plans, dory_halo_wire_ids
            ctx.preallocate()
            g = self.views[r]
            if g["localVtxCnt"]:
                for (l, d), t in self.tab.items():
                    (sl, sn), _, _ = _src(l, d)
                    ctx.upload(sl, sn, t[g["localToGlobal"]])
                    assert _poison_padding(ctx, sl, sn) == ctx.info(sl, sn)[2] - DIMS[l]
            self.ctxs.append(ctx)

    def lists(self, r, d):
        return self.views[r]["fwdLists" if d == 0 else "bwdLists"]

    def ghosts(self, r, d):
        return self.views[r]["srcGhost" if d == 0 else "dstGhost"]

    def sent(self, r, l, d, max_msg=0):
        """[(receiver, bytes)]: what the reference's sender loop on rank r sends for the exchange (l, d)"""
        g = self.views[r]
        return sm.send_messages(r, self.lists(r, d), g["localToGlobal"], self.tab[(l, d)][g["localToGlobal"]], DIMS[l], _src(l, d)[2], d, max_msg)

    def inbox(self, r, l, d, max_msg=0):
        """per sender, the messages rank r receives for the exchange (l, d)"""
        return [[m for (q, m) in self.sent(s, l, d, max_msg) if q == r] if s != r else [] for s in range(self.P)]

    def close(self):
        for c in self.ctxs:
            c.close()


_RANKS = {}


@pytest.fixture(scope="module")
def ranks(da):
    def get(case, direct=0):
        if (case, direct) not in _RANKS:
            _RANKS[(case, direct)] = Ranks(da, case, direct)
        return _RANKS[(case, direct)]
    yield get
    for v in _RANKS.values():
        v.close()
    _RANKS.clear()


def _short_last_batch(counts):
    """a batch size that leaves some peer a short last message (2 where no peer gets more than two rows)"""
    for b in (4, 5, 3, 7, 2):
        if any(c > b and c % b for c in counts):
            return b
    return 2


def _check_pack(ctx, layer, direction, name, max_msg, want, what):
    """layout + pack of one exchange against the messages `want` = [(receiver, bytes)] of the restatement"""
    import torch
    msgs, total = ctx.scatter_msgs_layout(layer, direction, name, max_msg)
    assert len(msgs) == len(want), (what, len(msgs), len(want))
    end = 0
    for (peer, first, rows, off, nbytes), (q, m) in zip(msgs, want):
        assert peer == q and nbytes == len(m) and off % 16 == 0 and off == (end + 15) // 16 * 16, (what, peer, q, off, end)
        assert rows == struct.unpack_from("<I", m, 12)[0]
        end = off + nbytes
    assert total == end, (what, total, end)
    buf = torch.full((total + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()       # (torch's fill runs on torch's stream, the pack on the context's non-blocking one)
    assert buf.data_ptr() % 16 == 0
    ctx.scatter_msgs_pack(layer, direction, buf.data_ptr(), name, max_msg)
    ctx.sync()
    got = buf.cpu().numpy()
    assert (got[total:] == 0xA5).all(), (what, "bytes behind total_bytes")
    end = 0
    for (peer, first, rows, off, nbytes), (q, m) in zip(msgs, want):
        assert not got[end:off].any(), (what, "bytes between the messages", end, off)
        assert got[off:off + nbytes].tobytes() == m, (what, "message for", peer, "rows", rows)
        assert not np.isnan(got[off + 28:off + nbytes].view(np.float32)).any(), (what, "NaN in a message")
        end = off + nbytes
    return msgs, total


# ---- 1. pack ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
def test_pack_is_the_senders_bytes(da, ranks, case):
    R = ranks(case)
    empty_senders = 0
    for r, ctx in enumerate(R.ctxs):
        for l in range(1, len(WIDTHS) + 1):
            rec = 4 + 4 * DIMS[l]
            for d in (da.FORWARD, da.BACKWARD):
                counts = [len(x) for x in R.lists(r, d)]
                for max_msg in (0, 28 + rec, 28 + 3 * rec, 28 + _short_last_batch(counts) * rec + 3):
                    want = R.sent(r, l, d, max_msg)
                    msgs, total = _check_pack(ctx, l, d, None, max_msg, want, (case, r, DIMS[l], d, max_msg))
                    if sum(counts) == 0:
                        assert msgs == [] and total == 0
                        empty_senders += 1
                    if max_msg == 28 + rec:
                        assert len(msgs) == sum(counts)
    if case == "parts_toy40_p3_empty":
        assert empty_senders, "a rank that sends nothing"


def test_pack_gat_prototype_and_multi_head_tensors_by_name(da):
    from helpers import _poison_padding
    pobjs, parts = _golden(da, "parts_toy60_p2")
    V = len(parts)
    rng = np.random.default_rng(3)
    for r, part in enumerate(pobjs):
        g = part.view()
        # the GAT prototype: forward z@(layer-1) -> fg_z@(layer-1), backward grad@(layer-1) -> bg_d@(layer-1): messages name layer - 1
        ctx = da.Context(0)
        ctx.configure(da.GAT, [8, 41, 5], V, r, 2)
        part.upload(ctx, parts)
        ctx.preallocate()
        for layer in (1, 2):
            for d, nm in ((da.FORWARD, "z"), (da.BACKWARD, "grad")):
                cols = ctx.info(layer - 1, nm)[1]
                x = rng.standard_normal((int(g["localVtxCnt"]), cols)).astype(np.float32)
                ctx.upload(layer - 1, nm, x)
                _poison_padding(ctx, layer - 1, nm)
                lists = g["fwdLists" if d == 0 else "bwdLists"]
                for max_msg in (0, 28 + 3 * (4 + 4 * cols)):
                    want = sm.send_messages(r, lists, g["localToGlobal"], x, cols, layer - 1, d, max_msg)
                    _check_pack(ctx, layer, d, None, max_msg, want, ("gat", r, layer, d, max_msg))
        ctx.close()
        # the multi-head GAT's backward exchanges, by name: "do" and "st" with the backward plan, messages name the tensor's layer
        ctx = da.Context(0)
        ctx.configure(da.GATMH, [8, 16, 4], V, r, 2)
        ctx.gatmh_heads([2, 2])
        part.upload(ctx, parts)
        ctx.preallocate()
        for layer in (0, 1):
            for nm in ("do", "st"):
                cols = ctx.info(layer, nm)[1]
                x = rng.standard_normal((int(g["localVtxCnt"]), cols)).astype(np.float32)
                ctx.upload(layer, nm, x)
                _poison_padding(ctx, layer, nm)
                for max_msg in (0, 28 + 3 * (4 + 4 * cols)):
                    want = sm.send_messages(r, g["bwdLists"], g["localToGlobal"], x, cols, layer, da.BACKWARD, max_msg)
                    _check_pack(ctx, layer, da.BACKWARD, nm, max_msg, want, ("gatmh", r, layer, nm, max_msg))
        ctx.close()


# ---- 2. deliver --------------------------------------------------------------------------------------------------------------------
def _dense_raw(da, R, r, l, d):
    """the raw ghost rows the dense exchange leaves on rank r: the split unpack (exact width: [0, cols) from the buffer, zeros into
    the padding -- the bits of the padded form, tests/test_gpu_halo_exact_rows.py) of the rows in plan order"""
    import torch
    ctx = R.ctxs[r]
    (_, _), (gl, gn), _ = _src(l, d)
    gv = np.concatenate([R.views[q]["localToGlobal"][R.lists(q, d)[r]] if q != r else np.zeros(0, np.uint32) for q in range(R.P)]).astype(np.int64)
    wire = R.tab[(l, d)][gv].reshape(-1)
    _fill_nan(ctx, gl, gn)
    buf = torch.from_numpy(np.concatenate([wire, np.zeros(4, np.float32)])).cuda()
    torch.cuda.synchronize()
    ctx.set_option("halo_exact_rows", 1)
    ctx.halo_unpack(l, d, buf.data_ptr())
    raw = _raw_rows(ctx, gl, gn)
    ctx.set_option("halo_exact_rows", 0)
    return raw


def _deliver_and_check(da, R, r, l, d, calls, dense, what):
    """NaN everywhere, the calls' messages, finish: every ghost row written once, raw rows = the dense exchange's, rows = the owners'"""
    ctx = R.ctxs[r]
    (_, _), (gl, gn), _ = _src(l, d)
    G = len(R.ghosts(r, d))
    _fill_nan(ctx, gl, gn)
    for msgs in calls:
        ctx.scatter_msgs_deliver(msgs)
    assert ctx.scatter_msgs_finish(l, d) == (G, 0, 0), what
    raw = _raw_rows(ctx, gl, gn)
    assert not np.isnan(raw).any(), (what, "a ghost row was not written")
    assert np.array_equal(_bits(raw), _bits(dense)), (what, "raw ghost rows against the dense exchange's")
    assert np.array_equal(_bits(ctx.download(gl, gn)), _bits(R.tab[(l, d)][R.ghosts(r, d).astype(np.int64)])), (what, "ghost rows against the owners' rows")


def _variants(R, r, l, d, rng):
    """name -> the deliver calls (lists of messages) of one round"""
    rec = 4 + 4 * DIMS[l]
    whole = [m for per in R.inbox(r, l, d) for m in per]
    cut3 = R.inbox(r, l, d, 28 + 3 * rec)
    flat3 = [m for per in cut3 for m in per]
    inter = [per[i] for i in range(max([len(p) for p in cut3] + [0])) for per in cut3 if i < len(per)]
    return {
        "all_in_one_call": [whole],
        "one_message_per_call": [[m] for m in flat3],
        "records_shuffled": [[sm.shuffled(m, rng) for m in whole]],
        "recut_1_and_7": [sm.recut(whole[:1], 1) + sm.recut(whole[1:], 7)],
        "senders_interleaved": [inter],
        "reversed_messages": [flat3[::-1]],
    }


@pytest.mark.parametrize("direct", (0, 1))
@pytest.mark.parametrize("case", CASES)
def test_deliver_lands_the_owners_rows(da, ranks, case, direct):
    R = ranks(case, direct)
    rng = np.random.default_rng(11)
    ran = set()
    for r in range(R.P):
        for li, l in enumerate(range(1, len(WIDTHS) + 1)):
            for d in (da.FORWARD, da.BACKWARD):
                if len(R.ghosts(r, d)) == 0:
                    continue
                dense = _dense_raw(da, R, r, l, d)
                var = _variants(R, r, l, d, rng)
                names = sorted(var)
                # every variant at three widths (dword rows, rows narrower and wider than a 128-byte line, none a multiple of 4);
                # at the others the plain round and one more, in turn
                pick = names if DIMS[l] in (1, 41, 130) else ["all_in_one_call", names[(li + d + r) % len(names)]]
                for nm in pick:
                    _deliver_and_check(da, R, r, l, d, var[nm], dense, (case, direct, r, DIMS[l], d, nm))
                    ran.add(nm)
    assert ran == set(_variants(R, 0, 1, 0, rng)) or case == "parts_toy40_p3_empty"


def test_deliver_takes_the_device_packed_messages_and_names(da, ranks):
    """the bytes dory_scatter_msgs_pack wrote on the senders, delivered to the receivers (by (layer, dir) and by tensor name)"""
    import torch
    R = ranks("parts_toy60_p4_hash")
    l = 1 + WIDTHS.index(41)
    for d in (da.FORWARD, da.BACKWARD):
        (_, _), (gl, gn), _ = _src(l, d)
        inbox = [[] for _ in range(R.P)]
        for s, ctx in enumerate(R.ctxs):
            msgs, total = ctx.scatter_msgs_layout(l, d, None, 28 + 5 * (4 + 4 * 41))
            buf = torch.zeros(total + 16, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            ctx.scatter_msgs_pack(l, d, buf.data_ptr(), None, 28 + 5 * (4 + 4 * 41))
            ctx.sync()
            host = buf.cpu().numpy()
            for (peer, first, rows, off, nbytes) in msgs:
                inbox[peer].append(host[off:off + nbytes].copy())
        for r in range(R.P):
            if len(R.ghosts(r, d)):
                dense = _dense_raw(da, R, r, l, d)
                _deliver_and_check(da, R, r, l, d, [inbox[r]], dense, ("device-packed", r, d))
                _fill_nan(R.ctxs[r], gl, gn)
                R.ctxs[r].scatter_msgs_deliver(inbox[r], name=gn)
                assert R.ctxs[r].scatter_msgs_finish(gl, d, gn) == (len(R.ghosts(r, d)), 0, 0)
                assert np.array_equal(_bits(_raw_rows(R.ctxs[r], gl, gn)), _bits(dense))


# ---- 3. errors ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("direct", (0, 1))
def test_errors_are_reported_and_the_next_round_is_clean(da, ranks, direct):
    R = ranks("parts_toy60_p2", direct)
    r, l, d = 0, 1 + WIDTHS.index(41), da.FORWARD
    ctx = R.ctxs[r]
    (_, _), (gl, gn), hdr_layer = _src(l, d)
    ghosts = R.ghosts(r, d)
    G = len(ghosts)
    assert G >= 3
    dense = _dense_raw(da, R, r, l, d)
    whole = [m for per in R.inbox(r, l, d) for m in per]
    assert len(whole) == 1
    recv, snd, cnt, fd, lay, dr, rec = sm.parse(whole[0])
    assert (recv, fd, lay, dr, cnt) == (r, 41, hdr_layer, d, G)
    stored = np.arange(G)
    if direct:       # ghost slot k is stored at the row the wire order gives it
        order = R.pobjs[r].wire_order(R.parts, d)[0]
        stored = np.argsort(order)

    def msg(records, receiver=r, feat=41, layer=hdr_layer, direction=d):
        records = np.ascontiguousarray(records, np.uint32)
        return sm.header(receiver, snd, len(records), feat, layer, direction) + records.tobytes()

    def clean_round(what):
        _deliver_and_check(da, R, r, l, d, [whole], dense, what)

    def counted_round(records, want_counts, missing_slot, what):
        _fill_nan(ctx, gl, gn)
        ctx.scatter_msgs_deliver([msg(records)])
        rc, rows, unknown, dup = ctx.scatter_msgs_finish(l, d, check=False)
        assert (rc, rows, unknown, dup) == (ERR_COMM,) + want_counts, what
        assert "scatter_msgs_finish" in ctx.lib.dory_last_error(ctx.h).decode()
        raw = _raw_rows(ctx, gl, gn)
        keep = np.ones(G, bool)
        if missing_slot is not None:
            keep[stored[missing_slot]] = False
            assert np.isnan(raw[stored[missing_slot]]).all(), (what, "a row nobody sent was written")
        assert np.array_equal(_bits(raw[keep]), _bits(dense[keep])), (what, "the rows of known ids")
        clean_round((what, "next round"))

    clean_round("first")
    k = int(np.flatnonzero(ghosts == rec[2, 0])[0])                  # the ghost slot of the third record
    # an unknown id (a local vertex of the receiver): counted, never written; its own slot stays unwritten
    bad = rec.copy()
    bad[2, 0] = R.views[r]["localToGlobal"][0]
    assert bad[2, 0] not in ghosts
    counted_round(bad, (G - 1, 1, 0), k, "unknown id")
    bad[2, 0] = 0xFFFFFFF0
    counted_round(bad, (G - 1, 1, 0), k, "unknown id beyond every ghost")
    # a duplicate (the same record twice): one of them is written, the other counted
    counted_round(np.concatenate([rec, rec[2:3]]), (G, 0, 1), None, "duplicate")
    # one record missing
    counted_round(np.delete(rec, 2, axis=0), (G - 1, 0, 0), k, "one record missing")
    # refused before anything is enqueued: nothing is written, the text names the field
    for m, pat in ((msg(rec[:, :41], feat=40), "featDim 40"), (whole[0][:-4], "truncated"), (whole[0][:20], "truncated"),
                   (msg(rec, receiver=1), "receiver 1 is not this rank"), (b"0000000" + whole[0][7:], "receiver field"),
                   (msg(rec, layer=99), "layer 99 out of range"), (msg(rec, direction=2), "dir 2")):
        _fill_nan(ctx, gl, gn)
        with pytest.raises(da.DoryError, match=r"error -1.*" + pat):
            ctx.scatter_msgs_deliver([whole[0][:28] + whole[0][28:], m] if pat != "truncated" else [m])
        rc, rows, unknown, dup = ctx.scatter_msgs_finish(l, d, check=False)
        assert (rc, rows, unknown, dup) == (ERR_COMM, 0, 0, 0), pat
        assert np.isnan(_raw_rows(ctx, gl, gn)).all(), (pat, "a refused call wrote ghost rows")
        clean_round((pat, "next round"))
    with pytest.raises(da.DoryError, match="error -1"):
        ctx.scatter_msgs_deliver([])
    # ids that are not ascending are refused, and the tables stay as they were
    g = R.views[r]
    with pytest.raises(da.DoryError, match="error -1.*not ascending"):
        ctx.halo_wire_ids(g["localToGlobal"], g["srcGhost"][::-1].copy(), g["dstGhost"])
    clean_round("after a refused dory_halo_wire_ids")


def test_delivery_into_layer_0_drops_the_cached_aggregate(da):
    """dory_scatter_msgs_deliver into fg@0 invalidates the cached ah@0 (option gcn_cache_ah0), as dory_halo_exchange(0, FORWARD) does:
    the next aggregation of layer 0 is computed, not answered from the cache"""
    pobjs, parts = _golden(da, "parts_toy60_p2")
    V, r = len(parts), 0
    g = pobjs[r].view()
    rng = np.random.default_rng(5)
    ctx = da.Context(0)
    ctx.configure(da.GCN, [6, 5, 3], V, r, 2)
    ctx.set_option("gcn_cache_ah0", 1)
    pobjs[r].upload(ctx, parts)
    ctx.preallocate()
    X = rng.standard_normal((V, 6)).astype(np.float32)
    ctx.upload(0, "x", X[g["localToGlobal"]])
    ctx.upload(0, "fg", X[g["srcGhost"]])
    ctx.aggregate(0, da.FORWARD)
    first = ctx.download(0, "ah")
    ctx.aggregate(0, da.FORWARD)
    skips = ctx.get_option("gcn_cache_ah0_skips")
    assert skips >= 1
    X2 = (X * 2).astype(np.float32)
    gv = g["srcGhost"]
    rec = np.empty((len(gv), 7), np.uint32)
    rec[:, 0] = gv
    rec[:, 1:] = X2[gv].view(np.uint32)
    ctx.scatter_msgs_deliver([sm.header(r, 1, len(gv), 6, 0, 0) + rec.tobytes()])
    assert ctx.scatter_msgs_finish(0, da.FORWARD) == (len(gv), 0, 0)
    ctx.aggregate(0, da.FORWARD)
    assert ctx.get_option("gcn_cache_ah0_skips") == skips, "the cached ah@0 was used after fg@0 changed"
    assert not np.array_equal(ctx.download(0, "ah"), first)
    ctx.close()


# ---- 4. the transport: processes on one device, gloo carries the messages as bytes ---------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _transport_worker(rank, world, port, case, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        sys.path.insert(0, ROOT)
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import torch
        import torch.distributed as dist
        import dorylus_amd as da
        dist.init_process_group("gloo", rank=rank, world_size=world)
        gnn = {"gcn": da.GCN, "gat": da.GAT, "gatmh": da.GATMH}[case["gnn"]]
        heads = case.get("heads")
        dims, V, E, epochs = case["dims"], case["V"], case["E"], case["epochs"]
        rng = np.random.default_rng(case["seed"])
        s, d = rng.integers(0, V, E), rng.integers(0, V, E)
        src, dst = np.concatenate([s, d]), np.concatenate([d, s])
        parts = rng.integers(0, world, V).astype(np.int32)
        X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
        labels = rng.integers(0, dims[-1], V).astype(np.uint32)
        L = len(dims) - 1
        Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]
        As = [(rng.standard_normal((dims[i + 1], 1)) / 2).astype(np.float32) for i in range(L)]
        if gnn == da.GATMH:      # the last layer keeps one copy of the class width per head
            zw = [dims[l + 1] * (heads[l] if l == L - 1 else 1) for l in range(L)]
            Ws = [(rng.standard_normal((dims[l], zw[l])) / np.sqrt(dims[l])).astype(np.float32) for l in range(L)]
            Al = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
            Ar = [(rng.standard_normal(zw[l]) * 0.3).astype(np.float32) for l in range(L)]
        wnames = {da.GCN: ("w",), da.GAT: ("w", "a_i"), da.GATMH: ("w", "a_l", "a_r")}[gnn]
        part = da.Partition.build(src, dst, parts, rank, world)
        g = part.view()

        def allreduce(buf):
            t = torch.from_numpy(buf.copy())
            dist.all_reduce(t)
            buf[:] = t.numpy()

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

        def run(transport, opts):
            ctx = da.Context(0)
            ctx.configure(gnn, dims, V, rank, world)
            if gnn == da.GATMH:
                ctx.gatmh_heads(heads)
            for k, v in dict(case.get("opts", {}), **opts).items():
                ctx.set_option(k, v)
            part.upload(ctx, parts)
            ctx.preallocate()
            if gnn == da.GCN:
                ctx.upload(0, "x", X[g["localToGlobal"]])
                if g["srcGhostCnt"]:
                    ctx.upload(0, "fg", X[g["srcGhost"]].reshape(g["srcGhostCnt"], dims[0]))
            else:
                ctx.upload(0, "h", X[g["localToGlobal"]])
            ctx.labels_upload(labels[g["localToGlobal"]])
            for l in range(L):
                ctx.weight_set(l, "w", Ws[l])
                if gnn == da.GAT:
                    ctx.weight_set(l, "a_i", As[l])
                if gnn == da.GATMH:
                    ctx.weight_set(l, "a_l", Al[l])
                    ctx.weight_set(l, "a_r", Ar[l])
            ctx.adam_config(0.01)
            stat = {"exchanges": 0, "msgs": 0, "bytes": 0}

            def exchange(msgs):
                """every message to its receiver as bytes; what arrived for this rank goes to dory_scatter_msgs_deliver before returning"""
                stat["exchanges"] += 1
                out = [[] for _ in range(world)]
                for peer, m in msgs:
                    out[peer].append(m.tobytes())
                    stat["msgs"] += 1
                    stat["bytes"] += m.size
                every = [None] * world
                dist.all_gather_object(every, out)
                mine = [m for s_ in range(world) if s_ != rank for m in every[s_][rank]]
                if mine:
                    ctx.scatter_msgs_deliver(mine)

            if transport == "scatter":
                ctx.set_scatter_transport(exchange, allreduce, case["max_msg"])
            else:
                ctx.set_host_transport(alltoallv, allreduce)
            eng = da.NativeEngine(ctx)
            eng.run(epochs)
            ctx.sync()
            out = {}
            for l in range(L + 1):
                for nm in ("ah", "h", "z", "aTg", "grad", "fg", "bg", "fg_z", "bg_d", "o", "t", "del", "der", "dz", "bg_do", "bg_st", "logits"):
                    try:
                        rows = ctx.info(l, nm)[0]
                    except da.DoryError:
                        continue
                    if rows:
                        out[(l, nm)] = ctx.download(l, nm)
            for l in range(L):
                for nm in wnames:
                    out[("W", l, nm)] = ctx.weight_get(l, nm)
                    out[("dW", l, nm)] = ctx.weight_grad_get(l, nm)
            eng.close()
            ctx.close()
            return out, stat

        def diff(a, b):
            return sorted(str(k) for k in set(a) | set(b) if k not in a or k not in b or not np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)))

        bad = {}
        host_exact, _ = run("host", {"halo_exact_rows": 1})
        scatter, stat = run("scatter", {})
        bad["scatter vs host transport with halo_exact_rows"] = diff(scatter, host_exact)
        no_overlap, _ = run("scatter", {"halo_overlap": 0})
        bad["scatter, halo_overlap 0 vs 1"] = diff(no_overlap, scatter)
        host_direct, _ = run("host", {"halo_direct_recv": 1})
        scatter_direct, _ = run("scatter", {"halo_direct_recv": 1})
        bad["scatter vs host transport, halo_direct_recv on both"] = diff(scatter_direct, host_direct)
        # GCN: h forward and grad backward between the layers; GAT: z and grad per layer; multi-head GAT: z forward per layer, and the
        # backward sweep's own "do" and "st" exchanges per layer
        n_exchanges = epochs * {da.GCN: 2 * (L - 1), da.GAT: 2 * L, da.GATMH: 3 * L}[gnn]
        ok = stat["exchanges"] == n_exchanges and len(scatter) > 2 * L and (stat["msgs"] > stat["exchanges"] or not g["localVtxCnt"])
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, {k: v for k, v in bad.items() if v}, ok, stat))
    except Exception:
        q.put((rank, traceback.format_exc(), False, None))


TRANSPORT_CASES = {
    "gcn": dict(gnn="gcn", dims=[64, 41, 7], V=1200, E=9000, seed=21, epochs=3, max_msg=28 + 50 * (4 + 4 * 41)),
    "gat": dict(gnn="gat", dims=[24, 16, 6], V=1200, E=9000, seed=22, epochs=1, max_msg=4096),
    # the 8-head extension: z forward, and the backward sweep's own "do" / "st" exchanges between its two phases
    "gatmh": dict(gnn="gatmh", dims=[40, 128, 41], heads=[8, 1], V=600, E=6000, seed=23, epochs=1, max_msg=8192, opts={"spmm_blk_nb": 8}),
}


@pytest.mark.parametrize("gnn,world", [("gcn", 2), ("gcn", 3), ("gat", 2), ("gat", 3), ("gatmh", 2)])
def test_scatter_transport_gives_the_host_transports_bits(gnn, world):
    import torch.multiprocessing as mp
    case = TRANSPORT_CASES[gnn]
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = _free_port()
    procs = [ctxm.Process(target=_transport_worker, args=(r, world, port, case, q)) for r in range(world)]
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
    for rank, bad, ok, stat in sorted(res, key=lambda t: t[0]):
        assert isinstance(bad, dict), f"rank {rank} failed:\n{bad}"
        assert not bad, (rank, bad)
        assert ok, (rank, stat)
