"""Option halo_direct_recv (include/dorylus_hip.h): ghost rows are stored in the order they arrive on the wire, the adjacency is
renumbered once on the host (dory_partition_wire_order), and an exchange whose wire width is the ghost tensor's ld lands in the
ghost tensor itself -- no receive buffer, no unpack.

  1. whole GCN epochs over the in-process device transport (the receiver pulls) on the golden partitions: the oracle's epochs
     by the existing criteria, ghost rows (downloaded in the caller's order) the owners' bits, one set of weight bits on every
     rank and with overlap on and off; under K1 (spmm_variant = 0: edges are walked in edge order) every bit of an option-0
     run; the counters;
  2. the same over the host transport (two processes, gloo);
  3. the GAT prototype and the 8-head GAT (its backward's do / st exchange lands directly too);
  4. twenty epochs back to back at P = 2 and P = 8;
  5. one context, no exchange: a renumbered adjacency through dory_graph_upload + dory_halo_plan, exact-arithmetic values
     (tests/aggregate_ref.py), K1 / K1b / K1s bit for bit the float64 reference; uploads, downloads, fills and
     dory_halo_unpack* of ghost tensors in the caller's order, the raw pointer in wire order;
  6. with halo_exact_rows: rows narrower than ld keep the staged path, rows of ld floats land directly; without a receive
     buffer a staged exchange fails with the documented message;
  7. refusals: the option after the upload, ranks that disagree, values outside {0, 1}.
No claim of bit equality with option 0 is made where K1s or K1b read ghost rows: they spread source rows over blocks by id,
and renumbered ghosts fall into other blocks."""
import os
import socket
import sys
import traceback

import numpy as np
import pytest

import aggregate_ref as ar
import halo_direct_ref as hd

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-4
KEYS = ("halo_direct_recvs", "halo_staged_recvs", "halo_recv_buf_bytes", "spmm_launches_k1", "spmm_launches_k1s", "spmm_launches_k1b")
DIMS = [20, 16, 6]


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _raw_rows(ctx, layer, name):
    """the raw ld-wide rows of a device tensor, through its dory_tensor_info pointer"""
    import ctypes as C
    rows, cols, ld, p = ctx.info(layer, name)
    out = np.empty((rows, ld), np.float32)
    if rows == 0:
        return out
    hip = C.CDLL("libamdhip64.so")
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    ctx.sync()
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(p), out.nbytes, 2) == 0
    return out


def _keep(setup, kept, extra=None):
    """run_local closes its contexts: read every rank's counters (and what `extra` wants of the context) just before that"""
    def wrapped(ctx, r, g):
        setup(ctx, r, g)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = {k: int(ctx.get_option(k)) for k in KEYS}
                if extra:
                    kept[r].update(extra(ctx, r, g))
            close()
        ctx.close = closing
    return wrapped


def _inputs(V, dims, seed=5):
    L = len(dims) - 1
    rng = np.random.default_rng(seed)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]
    return X, labels, Ws


def _gcn_setup(X, labels, Ws, dims):
    def setup(ctx, r, g):
        if g["localVtxCnt"]:
            ctx.upload(0, "x", X[g["localToGlobal"]])
        if g["srcGhostCnt"]:
            ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), dims[0]))       # the caller's order
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
    return setup


def _gcn_run(da, case, dims, epochs, opts, extra=None):
    from local_ranks import run_local
    pobjs, parts = hd.golden(da, case)
    L = len(dims) - 1
    X, labels, Ws = _inputs(len(parts), dims)
    dl = [(l, "ah") for l in range(L)] + [(l, nm) for l in range(L - 1) for nm in ("h", "aTg", "bg")] + [(l, nm) for l in range(1, L) for nm in ("grad", "fg")]
    kept = {}
    out = run_local(da, pobjs, parts, dims, da.GCN, epochs, _keep(_gcn_setup(X, labels, Ws, dims), kept, extra), opts, downloads=dl)
    return out, kept


_ORACLE = {}


def _oracle(da, case, dims, epochs):
    """the oracle's epochs of a case, computed once and shared"""
    key = (case, tuple(dims), epochs)
    if key not in _ORACLE:
        from test_gpu_local_transport import _oracle_epochs
        pobjs, parts = hd.golden(da, case)
        gs = [p.view() for p in pobjs]
        X, labels, Ws = _inputs(len(parts), dims)
        _ORACLE[key] = (gs, pobjs) + tuple(_oracle_epochs(gs, parts, X, labels, Ws, epochs))
    return _ORACLE[key]


def _direct_counters(kept, P, what):
    assert set(kept) == set(range(P)), what
    for r in range(P):
        assert kept[r]["halo_staged_recvs"] == 0 and kept[r]["halo_recv_buf_bytes"] == 0, (what, r, kept[r])
    assert sum(kept[r]["halo_direct_recvs"] for r in range(P)) > 0, (what, kept)


# ---- 1. GCN over the in-process device transport ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", hd.GOLDEN)
def test_local_transport_gcn_epochs_direct_recv(da, case):
    from test_gpu_local_transport import _check_vs_oracle, _same_bits
    epochs, L = 3, len(DIMS) - 1
    gs, _, T, dW, Wo = _oracle(da, case, DIMS, epochs)
    P = len(gs)
    for opts in ({"spmm_variant": 0}, {"spmm_blk_nb": 8}):
        runs = []
        for overlap in (1, 0):
            out, kept = _gcn_run(da, case, DIMS, epochs, dict(opts, halo_overlap=overlap, halo_direct_recv=1))
            _check_vs_oracle(out, gs, T, dW, Wo, L, (case, opts, overlap, "direct"))      # ghost rows: the owners' bits, caller order
            _direct_counters(kept, P, (case, opts, overlap))
            for r in range(P):      # every exchange of every rank: 2 per epoch (h0 forward, grad1 backward)
                assert kept[r]["halo_direct_recvs"] == 2 * epochs, (case, r, kept[r])
            runs.append((out, kept))
        _same_bits(runs[0][0], runs[1][0], (case, opts, "direct, overlap on / off"))
        if opts.get("spmm_variant") == 0:      # K1 walks a row's edges in edge order: renumbered ghosts change no sum
            out0, kept0 = _gcn_run(da, case, DIMS, epochs, dict(opts, halo_overlap=1, halo_direct_recv=0))
            _same_bits(runs[0][0], out0, (case, "K1: halo_direct_recv 1 / 0"))
            for k in (runs[0][1], kept0):
                ran = [r for r in range(P) if gs[r]["localVtxCnt"]]
                assert all(k[r]["spmm_launches_k1"] > 0 and k[r]["spmm_launches_k1s"] == 0 and k[r]["spmm_launches_k1b"] == 0 for r in ran), (case, k)
            for r in range(P):      # option 0 keeps its receive buffer and its unpack
                assert kept0[r]["halo_direct_recvs"] == 0 and kept0[r]["halo_staged_recvs"] == 2 * epochs, (case, r, kept0[r])
            assert sum(kept0[r]["halo_recv_buf_bytes"] for r in range(P)) > 0


def test_hash_partition_is_renumbered(da):
    """the case above cannot pass vacuously: on parts_toy60_p4_hash the wire order is not the identity, on any rank or side"""
    pobjs, parts = hd.golden(da, "parts_toy60_p4_hash")
    for part in pobjs:
        for direction in (0, 1):
            order, _ = part.wire_order(parts, direction)
            assert order.size and not np.array_equal(order, np.arange(order.size)), "order == arange"


# ---- 2. the host transport (worker pattern of tests/test_gpu_halo_exact_rows.py) ---------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, direct, case, epochs, q):
    try:
        os.environ["MASTER_ADDR"] = "127.0.0.1"
        os.environ["MASTER_PORT"] = str(port)
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        for p in (ROOT, os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
            sys.path.insert(0, p)
        import torch
        import torch.distributed as dist
        import dorylus_amd as da
        dist.init_process_group("gloo", rank=rank, world_size=world)
        pobjs, parts = hd.golden(da, case)
        part, g = pobjs[rank], pobjs[rank].view()
        X, labels, Ws = _inputs(len(parts), DIMS)
        L = len(DIMS) - 1
        ctx = da.Context(0)
        ctx.configure(da.GCN, DIMS, len(parts), rank, world)
        ctx.set_option("spmm_variant", 0)
        ctx.set_option("halo_direct_recv", direct)
        part.upload(ctx, parts)
        ctx.preallocate()
        _gcn_setup(X, labels, Ws, DIMS)(ctx, rank, g)
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
        eng.run(epochs)
        stats = (ctx.train_stat(), ctx.train_stat_global())
        ctx.sync()
        res = {"counters": {k: int(ctx.get_option(k)) for k in KEYS}, "tensors": {}, "stats": stats,
               "W": [{"w": ctx.weight_get(l)} for l in range(L)], "dW": [{"w": ctx.weight_grad_get(l)} for l in range(L)]}
        for l, nm in ((0, "ah"), (1, "ah"), (0, "h"), (0, "aTg"), (1, "grad"), (1, "fg"), (0, "bg")):
            if ctx.info(l, nm)[0]:
                res["tensors"][(l, nm)] = ctx.download(l, nm)
        eng.close()
        ctx.close()
        dist.barrier()
        dist.destroy_process_group()
        q.put((rank, res))
    except Exception:
        q.put((rank, traceback.format_exc()))


def _host_transport_run(direct, case, epochs):
    import torch.multiprocessing as mp
    world = 2
    ctxm = mp.get_context("spawn")
    q = ctxm.Queue()
    port = _free_port()
    procs = [ctxm.Process(target=_worker, args=(r, world, port, direct, case, epochs, q)) for r in range(world)]
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
    return {"tensors": [r["tensors"] for _, r in res], "weights": [r["W"] for _, r in res], "wgrads": [r["dW"] for _, r in res],
            "stats": [r["stats"] for _, r in res]}, {rank: r["counters"] for rank, r in res}


def test_host_transport_gcn_epochs_direct_recv(da):
    """two processes on one GPU, the bytes over gloo: the host-to-device copy of the received rows targets the ghost tensor"""
    from test_gpu_local_transport import _check_vs_oracle, _same_bits
    case, epochs = "parts_toy60_p2", 3
    gs, _, T, dW, Wo = _oracle(da, case, DIMS, epochs)
    out, kept = _host_transport_run(1, case, epochs)
    _check_vs_oracle(out, gs, T, dW, Wo, len(DIMS) - 1, (case, "host transport, direct"))
    _direct_counters(kept, 2, "host transport")
    out0, kept0 = _host_transport_run(0, case, epochs)
    _same_bits(out, out0, "host transport, K1: halo_direct_recv 1 / 0")
    for r in (0, 1):
        assert kept[r]["halo_direct_recvs"] == 2 * epochs and kept[r]["spmm_launches_k1"] > 0 and kept[r]["spmm_launches_k1s"] == 0, kept
        assert kept0[r]["halo_direct_recvs"] == 0 and kept0[r]["halo_staged_recvs"] == 2 * epochs and kept0[r]["halo_recv_buf_bytes"] > 0, kept0


# ---- 3. the GAT prototype and the 8-head GAT ---------------------------------------------------------------------------------
def test_local_transport_gat_prototype_direct_recv(da):
    """the GAT prototype as tests/test_gpu_local_transport.py checks it, on the one of its two goldens whose wire order is a
    real permutation (a rank of parts_toy60_p2 has a single peer: its rows arrive in slot order).  parts_toy60_p4_hash is not
    a case here: the prototype's aTg@0 misses the element-wise criterion on it with the option OFF already (measured: 2.57
    times the bound with option 0, 1.84 with option 1, 2.58 under K1 either way; max-norm 1.7e-6) -- a property of that graph
    and the prototype's fp32 sums that this option neither causes nor cures.  Since established as rounding on a cancelling
    sum, not a kernel error: the fp32 C oracle's own epoch misses the same criterion there against a float64 epoch (1.2 times,
    tests/test_gat_stage_reference.py), and stage by stage on the oracle epoch's inputs the GPU's aTg@0 sits at 0.27 of the
    bound derived from the magnitudes summed (0.009 of this criterion; the oracle: 0.29 and 0.018) --
    tests/test_gpu_gat_stage.py::test_open_case_p4_hash_per_stage is that graph's GAT-prototype coverage"""
    from helpers import assert_parity, oracle_gat_epoch_parts
    from local_ranks import run_local
    from test_gpu_local_transport import _same_bits
    case, dims, L = "parts_toy97_p8_und", DIMS, 2
    assert not np.array_equal(hd.golden(da, case)[0][0].wire_order(hd.golden(da, case)[1], 0)[0], np.arange(int(hd.golden(da, case)[0][0].view()["srcGhostCnt"])))
    runs = []
    for overlap in (1, 0):
        pobjs, parts = hd.golden(da, case)
        gs = [p.view() for p in pobjs]
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
        out = run_local(da, pobjs, parts, dims, da.GAT, 1, _keep(setup, kept), {"spmm_blk_nb": 8, "halo_overlap": overlap, "halo_direct_recv": 1},
                        downloads=dl)
        _direct_counters(kept, len(gs), ("GAT prototype", overlap))
        T, dWs, das = oracle_gat_epoch_parts(gs, parts, H0, labels, Ws, As)
        g2row = {}
        for r, g in enumerate(gs):
            t = out["tensors"][r]
            for i, gv in enumerate(g["localToGlobal"]):
                g2row[int(gv)] = [(t[(l, "z")][i],) for l in range(L)]
        for r, g in enumerate(gs):
            t = out["tensors"][r]
            for l in range(L):
                for nm in ("z", "ah", "aTg"):
                    assert_parity(t[(l, nm)], T[r][f"{nm}{l}"], (case, r, l, nm))
                if g["srcGhostCnt"]:
                    assert_parity(t[(l, "fg_z")], T[r][f"fg_z{l}"], (case, r, l, "fg_z"))
                    assert np.array_equal(_bits(t[(l, "fg_z")]), _bits(np.stack([g2row[int(gv)][l][0] for gv in g["srcGhost"]]))), (r, l, "fg_z bits")
        for l in range(L):
            assert_parity(out["wgrads"][0][l]["w"], dWs[l], (case, "dW", l))
        runs.append(out)
    _same_bits(runs[0], runs[1], (case, "GAT prototype direct, overlap on / off"))


def test_local_transport_gat_mh_direct_recv(da):
    """the 8-head extension at P = 4 (owners interleaved: parts = a permutation modulo P): z forward, do and st between the two
    phases of the backward sweep -- all through exchange_rows, all at their tensors' ld"""
    import gat_mh_oracle as go
    import partition_oracle as po
    from helpers import rel_err
    from local_ranks import run_local
    P, dims, heads, V, E = 4, [40, 128, 41], [8, 1], 240, 2600
    rng = np.random.default_rng(17)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    d[:200] = 7
    s[200:400] = 13
    parts = (rng.permutation(V) % P).astype(np.int32)
    g_all = po.preprocess(s, d, np.zeros(V, np.int64), 0, 1)
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
        for l, (W, al, a_r) in enumerate(params):
            ctx.weight_set(l, "w", W)
            ctx.weight_set(l, "a_l", al)
            ctx.weight_set(l, "a_r", a_r)
    pobjs = [da.Partition.build(s.astype(np.uint32), d.astype(np.uint32), parts, r, P) for r in range(P)]
    assert all(not np.array_equal(o, np.arange(o.size)) for p in pobjs for o in (p.wire_order(parts, 0)[0], p.wire_order(parts, 1)[0]))
    dl = [(l, nm) for l in range(2) for nm in ("z", "o", "do", "st", "t", "del", "der", "dz", "fg_z", "bg_do", "bg_st")] + [(1, "logits")]
    kept = {}
    out = run_local(da, pobjs, parts, dims, da.GATMH, 1, _keep(setup, kept), {"spmm_blk_nb": 8, "halo_direct_recv": 1}, downloads=dl,
                    pre=lambda c: c.gatmh_heads(heads), wnames=("w", "a_l", "a_r"))
    _direct_counters(kept, P, "8-head GAT")
    for r in range(P):      # per epoch: z of two layers forward, do and st of two layers backward
        assert kept[r]["halo_direct_recvs"] == 2 + 4, kept
    fws, Hs, loss, dlogits, grads = go.epoch(g_all, X, labels, [[p.astype(np.float64) for p in ps] for ps in params], heads)

    def gathered(layer, name):
        res = None
        for r, vw in enumerate(out["views"]):
            t = out["tensors"][r][(layer, name)]
            if res is None:
                res = np.zeros((V, t.shape[1]), np.float32)
            res[vw["localToGlobal"]] = t
        return res
    for l in range(2):
        assert rel_err(gathered(l, "z"), fws[l]["Z"]) < RTOL, (l, "z")
        assert rel_err(gathered(l, "o"), fws[l]["O"]) < RTOL, (l, "o")
        for nm, key in (("t", "t"), ("del", "d_el"), ("der", "d_er"), ("dz", "dZ")):
            assert rel_err(gathered(l, nm), grads[l][key]) < 5e-4, (l, nm)
        for nm, key in (("w", "dW"), ("a_l", "da_l"), ("a_r", "da_r")):
            assert rel_err(out["wgrads"][0][l][nm].reshape(np.shape(grads[l][key])), grads[l][key]) < 5e-4, (l, nm)
            for r in range(1, P):
                assert np.array_equal(out["wgrads"][r][l][nm], out["wgrads"][0][l][nm]), (l, nm, r)
        # ghost rows, downloaded in the caller's order, are the owners' rows bit for bit -- the backward's do / st included
        for ghost, own, side in (("fg_z", "z", "srcGhost"), ("bg_do", "do", "dstGhost"), ("bg_st", "st", "dstGhost")):
            whole = gathered(l, own)
            for r, vw in enumerate(out["views"]):
                if len(vw[side]):
                    assert np.array_equal(_bits(out["tensors"][r][(l, ghost)]), _bits(whole[vw[side]])), (l, ghost, r)
    assert rel_err(gathered(1, "logits"), Hs[2]) < RTOL


# ---- 4. twenty epochs back to back -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy97_p8_und"])
def test_local_transport_twenty_epochs_direct_recv(da, case):
    """40 exchanges and 40 gradient sums per rank over the two-deep event rings, the receivers pulling: nothing times out,
    overlap on and off end in the same bits, the 20th epoch is the oracle's 20th"""
    from helpers import rel_err
    from test_gpu_local_transport import _same_bits
    gs, _, T, dW, Wo = _oracle(da, case, DIMS, 20)
    _, _, Ws = _inputs(len(hd.golden(da, case)[1]), DIMS)
    runs = []
    for overlap in (1, 0):
        out, kept = _gcn_run(da, case, DIMS, 20, {"spmm_blk_nb": 8, "halo_overlap": overlap, "halo_direct_recv": 1})
        assert all(np.isfinite(w[l]["w"]).all() for w in out["weights"] for l in range(2))
        assert np.abs(out["weights"][0][0]["w"] - Ws[0]).max() > 1e-3
        _direct_counters(kept, len(gs), (case, overlap))
        assert all(kept[r]["halo_direct_recvs"] == 40 for r in range(len(gs))), kept
        assert all(g["timeouts"] >= 0 and g["ungated_launches"] >= 0 for g in out["gates"])      # (read as the existing test reads them: the ranks share the device's CUs)
        runs.append(out)
    _same_bits(runs[0], runs[1], (case, "20 epochs direct, overlap on / off"))
    for l in range(2):
        assert rel_err(runs[0]["weights"][0][l]["w"], Wo[l]) < 5e-4, l       # (20 Adam steps of fp32 rounding apart)


# ---- 5. one context, no exchange -----------------------------------------------------------------------------------------------
def _single_ctx(da, part, parts, r, P, F, options, seed):
    """a direct dory_graph_upload caller: the renumbered adjacency (exact values substituted) and both plans, recv_slots = order"""
    from helpers import make_ctx
    v = part.view()
    g = ar.substitute_exact_values({k: v[k] for k in ("localVtxCnt", "globalVtxCnt", "srcGhostCnt", "dstGhostCnt", "colPtr", "rowIdx", "cscVal",
                                                        "rowPtr", "colIdx", "csrVal", "norm")}, seed=seed)
    orders = [part.wire_order(parts, d)[0] for d in (0, 1)]
    ctx = make_ctx(da, hd.wired_graph(g, orders), [F, F, 3], int(v["globalVtxCnt"]), node_id=r, num_nodes=P, options=options)
    ctx.halo_plan(da.FORWARD, v["fwdLists"], part.recv_plan(parts, 0))
    ctx.halo_plan(da.BACKWARD, v["bwdLists"], part.recv_plan(parts, 1))
    return ctx, g, orders


def test_single_context_wire_ordered_ghosts_exact(da):
    from helpers import splitmix_uniform
    from test_gpu_aggregate_stage import _aggregate_counted, _mirror_applies
    name, F, P = "parts_toy60_p4_hash", 64, 4
    pobjs, parts = hd.golden(da, name)
    k1_ran = 0
    for r, part in enumerate(pobjs):
        ctx, g, orders = _single_ctx(da, part, parts, r, P, F, {"spmm_blk_nb": 16, "halo_direct_recv": 1}, seed=r)
        N = int(g["localVtxCnt"])
        mirror_ok = _mirror_applies(ctx)
        for direction, (layer, dirn, xl_name, xg_name, out_name) in (("fwd1", (1, da.FORWARD, (0, "h"), (1, "fg"), (1, "ah"))),
                                                                      ("bwd", (1, da.BACKWARD, (1, "grad"), (0, "bg"), (0, "aTg")))):
            d = 0 if direction == "fwd1" else 1
            order = orders[d]
            ptr, idx, val, ghosts = ar.side(g, direction)               # the caller's numbering: the reference is computed on it
            assert ghosts > 0 and not np.array_equal(order, np.arange(ghosts))
            x, xg = ar.features(g, direction, F, True, seed=r)
            ar.exact_ok(ptr, idx, val, g["norm"], x, xg, 1)
            ref = ar.aggregate(ptr, idx, val, g["norm"], x, xg, 1)
            ref32 = ref.astype(np.float32)
            assert (ref32.astype(np.float64) == ref).all()
            ctx.upload(*xl_name, x)
            ctx.upload(*xg_name, xg)                                    # the caller's order
            assert np.array_equal(_bits(ctx.download(*xg_name)), _bits(xg)), (r, direction, "download returns what was uploaded")
            raw = _raw_rows(ctx, *xg_name)
            assert np.array_equal(_bits(raw[:, :F]), _bits(xg[order])), (r, direction, "the raw pointer's rows are the wire order")
            idx_wire = hd.renumber(idx, N, order)
            stats = ar.AdjStats(N, ptr, idx_wire)
            for family in ("k1", "k1b", "k1s"):
                ctx.set_option("spmm_variant", ar.FAMILIES[family])
                ctx.upload(*out_name, np.full((N, F), np.nan, np.float32))
                moved = _aggregate_counted(ctx, da, layer, dirn)
                got = ctx.download(*out_name)
                bad = np.nonzero(((got + np.float32(0)).view(np.uint32) != (ref32 + np.float32(0)).view(np.uint32)).any(axis=1))[0]
                assert bad.size == 0, (r, direction, family, "rows that differ", bad[:8].tolist())
                assert sorted(moved.values()) == [0, 0, 1], (r, direction, family, moved)
                if family == "k1":
                    assert moved["k1"] == 1, moved
                    k1_ran += 1
                elif mirror_ok:
                    rec = ar.dispatch(N, ghosts, F, ptr, idx_wire, dict(ar.DEFAULTS, spmm_blk_nb=16, spmm_variant=ar.FAMILIES[family], layout_loader=1), stats=stats)
                    print(r, direction, family, "ran", moved, "mirror", rec["family"])
                    assert moved[rec["family"]] == 1, (r, direction, family, moved, rec["family"])
            ctx.set_option("spmm_variant", 2)
            # dory_tensor_fill_uniform: the caller-visible values of option 0, with and without global row ids
            gv = part.view()["srcGhost" if d == 0 else "dstGhost"]
            ctx.fill_uniform(*xg_name, 77, row_ids=gv)
            assert np.array_equal(_bits(ctx.download(*xg_name)), _bits(splitmix_uniform(77, gv, F))), (r, direction, "fill by global id")
            ctx.fill_uniform(*xg_name, 78)
            assert np.array_equal(_bits(ctx.download(*xg_name)), _bits(splitmix_uniform(78, np.arange(ghosts), F))), (r, direction, "fill by row")
            # dory_halo_unpack*: the caller's buffer in plan order, row r -> ghost row r
            import torch
            wire = np.random.default_rng([r, d]).standard_normal((ghosts, F)).astype(np.float32)
            buf = torch.from_numpy(wire).cuda()
            torch.cuda.synchronize()
            if d == 0:
                ctx.halo_unpack(1, da.FORWARD, buf.data_ptr())
            else:
                ctx.halo_unpack_tensor(0, "bg", da.BACKWARD, buf.data_ptr())
            assert np.array_equal(_bits(_raw_rows(ctx, *xg_name)[:, :F]), _bits(wire)), (r, direction, "unpack: row r to ghost row r")
            want = np.empty_like(wire)
            want[order] = wire
            assert np.array_equal(_bits(ctx.download(*xg_name)), _bits(want)), (r, direction, "unpacked rows in the caller's order")
        for k in ("halo_direct_recvs", "halo_staged_recvs", "halo_recv_buf_bytes"):      # nothing was exchanged, nothing allocated
            assert ctx.get_option(k) == 0, k
        ctx.close()
    assert k1_ran == 2 * P


def test_single_context_narrow_and_single_column_ghost_tensors(da):
    """uploads and downloads of ghost tensors whose rows are padded (41 of 64 floats) or a single float (ld = 1: the per-head
    tensors of a single head) go through the same permutation"""
    name, P = "parts_toy60_p4_hash", 4
    pobjs, parts = hd.golden(da, name)
    part, v = pobjs[1], pobjs[1].view()
    ctx, g, orders = _single_ctx(da, part, parts, 1, P, 41, {"halo_direct_recv": 1}, seed=1)
    G = int(v["srcGhostCnt"])
    x = np.random.default_rng(1).standard_normal((G, 41)).astype(np.float32)
    ctx.upload(1, "fg", x)
    assert np.array_equal(_bits(ctx.download(1, "fg")), _bits(x))
    raw = _raw_rows(ctx, 1, "fg")
    assert np.array_equal(_bits(raw[:, :41]), _bits(x[orders[0]])) and (raw[:, 41:] == 0).all()
    ctx.close()
    # a multi-head GAT context whose last layer has one head: fg_el / fg_er of one column
    from helpers import make_ctx
    gw = hd.wired_graph({k: v[k] for k in ("localVtxCnt", "globalVtxCnt", "srcGhostCnt", "dstGhostCnt", "colPtr", "rowIdx", "cscVal", "rowPtr",
                                            "colIdx", "csrVal", "norm")}, orders)
    c = da.Context(0)
    c.configure(da.GATMH, [8, 16, 4], int(v["globalVtxCnt"]), 1, P)
    c.gatmh_heads([2, 1])
    c.set_option("halo_direct_recv", 1)
    c.graph_upload(gw)
    c.preallocate()
    with pytest.raises(da.DoryError, match="dory_halo_plan"):      # the wire order is unknown before the plan
        c.upload(1, "fg_el", np.zeros((G, 1), np.float32))
    c.halo_plan(da.FORWARD, v["fwdLists"], part.recv_plan(parts, 0))
    c.halo_plan(da.BACKWARD, v["bwdLists"], part.recv_plan(parts, 1))
    assert c.info(1, "fg_el")[1:3] == (1, 1)
    e = np.arange(G, dtype=np.float32).reshape(G, 1) + 0.5
    c.upload(1, "fg_el", e)
    assert np.array_equal(c.download(1, "fg_el"), e)
    assert np.array_equal(_raw_rows(c, 1, "fg_el"), e[orders[0]])
    c.close()


# ---- 6. with halo_exact_rows ---------------------------------------------------------------------------------------------------
def test_exact_rows_narrow_tensors_stay_staged_wide_ones_land(da):
    """halo_exact_rows = 1 before the plan, layers of 41 and 128 floats: h0 / grad1 (41 of 64 floats) take the receive buffer and
    the unpack kernels (identity slots), h1 / grad2 (128 = ld) land in the ghost tensors"""
    from test_gpu_local_transport import _check_vs_oracle
    case, dims, epochs = "parts_toy60_p4_hash", [20, 41, 128, 6], 2
    gs, _, T, dW, Wo = _oracle(da, case, dims, epochs)

    def padding(ctx, r, g):
        if not g["srcGhostCnt"]:
            return {}
        raw = _raw_rows(ctx, 1, "fg")
        return {"pad_zero": bool((raw[:, 41:] == 0).all()), "pad_cols": raw.shape[1] - 41}
    for opts in ({"spmm_variant": 0}, {"spmm_blk_nb": 8}):
        out, kept = _gcn_run(da, case, dims, epochs, dict(opts, halo_exact_rows=1, halo_direct_recv=1), extra=padding)
        _check_vs_oracle(out, gs, T, dW, Wo, len(dims) - 1, (case, opts, "exact + direct"))      # ghost rows: the owners' bits
        for r in range(len(gs)):
            assert kept[r]["halo_staged_recvs"] == 2 * epochs and kept[r]["halo_direct_recvs"] == 2 * epochs, (r, kept[r])
            assert kept[r]["halo_recv_buf_bytes"] > 0 or not (gs[r]["srcGhostCnt"] or gs[r]["dstGhostCnt"]), (r, kept[r])
            if gs[r]["srcGhostCnt"]:
                assert kept[r]["pad_zero"] and kept[r]["pad_cols"] == 23, (r, kept[r])


def test_exact_rows_after_the_plan_fail_instead_of_allocating(da):
    pobjs, parts = hd.golden(da, "parts_toy60_p2")
    gs = [p.view() for p in pobjs]
    rng = np.random.default_rng(3)
    ctxs, H = [], []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GCN, [20, 41, 6], len(parts), r, 2)
        ctx.set_option("local_timeout_ms", 2000)
        ctx.set_option("halo_direct_recv", 1)
        part.upload(ctx, parts)
        ctx.preallocate()
        H.append(rng.uniform(-1, 1, (int(gs[r]["localVtxCnt"]), 41)).astype(np.float32))
        ctx.upload(0, "h", H[r])
        assert ctx.get_option("halo_recv_buf_bytes") == 0
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    for c in ctxs:
        c.set_option("halo_exact_rows", 1)
    for c in ctxs:
        with pytest.raises(da.DoryError, match=r"error -1.*halo_direct_recv.*halo_exact_rows = 1 before dory_halo_plan"):
            c.halo_exchange(1, da.FORWARD)
        assert c.get_option("halo_recv_buf_bytes") == 0 and c.get_option("halo_staged_recvs") == 0 and c.get_option("halo_rows_packed") == 0
    for c in ctxs:      # padded rows again: the exchange lands directly
        c.set_option("halo_exact_rows", 0)
    ctxs[0].halo_exchange(1, da.FORWARD)
    ctxs[1].halo_exchange(1, da.FORWARD)
    ctxs[0].sync()
    ctxs[1].sync()
    g2row = {int(gv): H[r][i] for r in (0, 1) for i, gv in enumerate(gs[r]["localToGlobal"])}
    for r in (0, 1):
        assert gs[r]["srcGhostCnt"] > 0
        assert np.array_equal(_bits(ctxs[r].download(1, "fg")), _bits(np.stack([g2row[int(gv)] for gv in gs[r]["srcGhost"]]))), r
        assert ctxs[r].get_option("halo_direct_recvs") == 1 and ctxs[r].get_option("halo_recv_buf_bytes") == 0
    for c in ctxs:
        c.close()


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
def test_option_values_and_time_of_setting(da):
    pobjs, parts = hd.golden(da, "parts_toy60_p2")
    for gnn in (da.GCN, da.GAT, da.GATMH):
        c = da.Context(0)
        assert c.get_option("halo_direct_recv") == 0
        for bad in (-1, 2, 7):
            with pytest.raises(da.DoryError, match="halo_direct_recv"):
                c.set_option("halo_direct_recv", bad)
        c.configure(gnn, [8, 16, 4], len(parts), 0, 2)
        c.set_option("halo_direct_recv", 1)
        c.set_option("halo_direct_recv", 0)
        c.set_option("halo_direct_recv", 1)
        assert c.get_option("halo_direct_recv") == 1
        for k in ("halo_direct_recvs", "halo_staged_recvs", "halo_recv_buf_bytes"):
            assert c.get_option(k) == 0
            with pytest.raises(da.DoryError):
                c.set_option(k, 1)
        pobjs[0].upload(c, parts)
        for v in (0, 1):      # the adjacency's numbering depends on it
            with pytest.raises(da.DoryError, match=r"error -1.*halo_direct_recv.*before the graph is uploaded"):
                c.set_option("halo_direct_recv", v)
        assert c.get_option("halo_direct_recv") == 1
        c.close()
    # a partition with ghosts cannot be renumbered without the parts vector
    c = da.Context(0)
    c.configure(da.GCN, DIMS, len(parts), 0, 2)
    c.set_option("halo_direct_recv", 1)
    with pytest.raises(da.DoryError, match="parts"):
        pobjs[0].upload(c)
    c.close()


def test_local_transport_refuses_ranks_that_disagree(da):
    """rank 0 with the option, rank 1 without: who pushes and who pulls is undefined -- the exchange fails at once with
    DORY_ERR_COMM naming both ranks, on either rank, before anything is enqueued or counted"""
    import time
    pobjs, parts = hd.golden(da, "parts_toy60_p2")
    ctxs = []
    for r, part in enumerate(pobjs):
        ctx = da.Context(0)
        ctx.configure(da.GCN, DIMS, len(parts), r, 2)
        ctx.set_option("local_timeout_ms", 2000)
        ctx.set_option("halo_direct_recv", 1 - r)
        part.upload(ctx, parts)
        ctx.preallocate()
        ctxs.append(ctx)
    da.Context.comm_init_local(ctxs)
    for r in (0, 1):
        t0 = time.perf_counter()
        with pytest.raises(da.DoryError, match=r"error -4.*halo_direct_recv.*rank %d has %d.*rank %d has %d" % (r, 1 - r, 1 - r, r)):
            ctxs[r].halo_exchange(1, da.FORWARD)
        assert time.perf_counter() - t0 < 1.0
        assert ctxs[r].get_option("halo_rows_packed") == 0 and ctxs[r].get_option("halo_direct_recvs") == 0 and ctxs[r].get_option("halo_staged_recvs") == 0
    for c in ctxs:
        c.close()
