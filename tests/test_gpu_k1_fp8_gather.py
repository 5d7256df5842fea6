"""dory_k1_fp8_gather (include/dorylus_hip.h; csrc/spmm_fp8.hip): K1's GCN aggregations on fp8 rows.  All with spmm_variant = 0 unless
a case says otherwise, so K1 runs.

  * the conversion kernel's shadow bytes and exponents are k1_fp8_rows' (the host statement of the format);
  * an aggregation with the mode on equals BIT FOR BIT the mode-0 aggregation of the dequantised rows, and the float64 aggregate of
    those rows within the K1 tolerances of tests/helpers.py -- one width per instantiation up to two gridDim.y slabs, on the 203-row
    graph of k1_bf16_wide_ref (ghost rows, multi-edges, self loops, degrees 0, 1, 3, 4, 5 and g - 1, g, g + 1 for every lane group),
    in one launch and in the two launches of the edge split, and with a row of LONG_ROW_CLAMP + LONG_ROW_CHUNK + 3 edges;
  * two ranks over the in-process transport, exchange in flight against halo_overlap = 0: the same bits; a short training run;
  * what is not taken (ld = 32, an aggregation K1s runs) and what is refused."""
import numpy as np
import pytest

import aggregate_ref as ar
import k1_bf16_wide_ref as kr

pytestmark = pytest.mark.gpu

WIDTHS = [64, 96, 128, 200, 300, 602, 1100, 2060]      # ld 64 .. 2080: (8,1,8) (16,1,8) (8,1,16) (16,1,16) (32,1,16) (64,1,16) (64,2,16) (64,2,16) x 2 slabs
TENSORS = {"fwd0": (0, "FORWARD", (0, "x"), (0, "fg"), (0, "ah")), "fwd1": (1, "FORWARD", (0, "h"), (1, "fg"), (1, "ah")),
           "bwd": (1, "BACKWARD", (1, "grad"), (0, "bg"), (0, "aTg"))}


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _raw(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _dequantise(q, e, cols):
    import torch
    return (torch.from_numpy(q[:, :cols].copy()).view(torch.float8_e4m3fn).to(torch.float32).numpy() *
            np.ldexp(np.float32(1), e.astype(np.int32) - 127)[:, None]).astype(np.float32)


def _aggregate(ctx, da, direction, mode, rows, shape):
    """upload the local and ghost rows, aggregate with `mode` into an output poisoned with NaN: (the output, what the counters moved by)"""
    layer, dirn, xl, xg, out = TENSORS[direction]
    N = shape[0]
    ctx.upload(xl[0], xl[1], rows[:N])
    if len(rows) > N:
        ctx.upload(xg[0], xg[1], rows[N:])
    ctx.upload(out[0], out[1], np.full(shape, np.nan, np.float32))
    ctx.k1_fp8_gather(mode)
    s0 = ctx.k1_fp8_gather_stats()
    ctx.aggregate(layer, getattr(da, dirn))
    s1 = ctx.k1_fp8_gather_stats()
    return ctx.download(out[0], out[1]), {k: s1[k] - s0[k] for k in s1}


@pytest.mark.parametrize("long_row", [False, True], ids=["short", "long_row"])
@pytest.mark.parametrize("F", WIDTHS)
def test_shadow_bytes_and_aggregate_bits(da, F, long_row):
    from helpers import assert_parity, make_ctx
    g = kr.graph203("real", long_row)
    N, ld = kr.N_ROWS, ar.pad_ld(F)
    ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), options={"spmm_variant": 0})
    for direction in ar.DIRECTIONS:
        ptr, idx, val, G = ar.side(g, direction)
        rng = np.random.default_rng([93, F, len(direction)])
        rows = (rng.uniform(-1, 1, (N + G, F)) * 2.0 ** rng.integers(-12, 12, (N + G, 1))).astype(np.float32)   # a scale of its own per row
        rows[5] = 0
        wq, we = da.k1_fp8_rows(rows, ld)
        deq = _dequantise(wq, we, F)
        want, moved = _aggregate(ctx, da, direction, 0, deq, (N, F))
        assert moved == dict.fromkeys(moved, 0)
        ref = ar.aggregate(ptr, idx, val, g["norm"], deq[:N], deq[N:], 1)
        for split in (0, 1):      # 1: the local-first copy in two launches (fwd1, bwd), the row split (fwd0)
            ctx.set_option("spmm_blk_force_split", split)
            got, moved = _aggregate(ctx, da, direction, 2, rows, (N, F))
            assert moved == {"fp8": 1, "other_family": 0, "no_form": 0, "rows_converted": N + G}, (F, direction, split, moved)
            q, e = ctx.k1_fp8_gather_download()
            assert q.shape == (N + G, ld) and np.array_equal(e, we) and np.array_equal(q, wq), (F, direction, np.argwhere(q != wq)[:4].tolist())
            bad = np.nonzero((_raw(got) != _raw(want)).any(axis=1))[0]
            assert bad.size == 0, (F, direction, split, "rows that differ from mode 0 on the dequantised rows", bad[:8].tolist(),
                                   got[bad[0], :4].tolist(), want[bad[0], :4].tolist())
            assert_parity(got, ref, (F, direction, split))
        ctx.set_option("spmm_blk_force_split", 0)
        if direction == "bwd":      # mode 1 leaves the backward aggregation alone
            got, moved = _aggregate(ctx, da, direction, 1, deq, (N, F))
            assert moved == dict.fromkeys(moved, 0) and np.array_equal(_raw(got), _raw(want))
    ctx.close()


DIMS = [100, 64, 41]      # 128-, 64- and 64-float rows
DOWNLOADS = [(l, nm) for l in range(2) for nm in ("ah", "z")] + [(0, "h"), (0, "aTg"), (1, "grad")]


def _two_ranks(da, overlap, mode, epochs=2):
    from local_ranks import run_local
    V, E = 600, 4000
    rng = np.random.default_rng(97)
    s, d = rng.integers(0, V, E), rng.integers(0, V, E)
    src, dst, parts = np.concatenate([s, d]), np.concatenate([d, s]), rng.integers(0, 2, V).astype(np.int32)
    X, labels = rng.uniform(-1, 1, (V, DIMS[0])).astype(np.float32), rng.integers(0, DIMS[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((DIMS[i], DIMS[i + 1])) / np.sqrt(DIMS[i])).astype(np.float32) for i in range(2)]
    kept = {}

    def setup(ctx, r, g):
        ctx.upload(0, "x", X[g["localToGlobal"]])
        ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), DIMS[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
        ctx.k1_fp8_gather(mode)
        close = ctx.close

        def closing():        # run_local closes its contexts: read the counters just before that
            if ctx.h:
                kept[r] = ctx.k1_fp8_gather_stats()
            close()
        ctx.close = closing

    out = run_local(da, [da.Partition.build(src, dst, parts, r, 2) for r in range(2)], parts, DIMS, da.GCN, epochs, setup,
                    {"spmm_variant": 0, "halo_overlap": overlap}, downloads=DOWNLOADS)
    return out, kept


def test_two_ranks_exchange_in_flight_same_bits_as_sequential(da):
    """two epochs on two ranks, mode 2: with the exchange in flight K1 sums the local-source edges beside it and goes on from those sums
    once the ghost rows are converted -- the bits of halo_overlap = 0, in every tensor, weight and weight gradient; and mode 2 is not mode 0"""
    seq, kseq = _two_ranks(da, 0, 2)
    ovl, kovl = _two_ranks(da, 1, 2)
    off, koff = _two_ranks(da, 1, 0)
    for r in range(2):
        for k in DOWNLOADS:
            assert np.isfinite(ovl["tensors"][r][k]).all() and np.array_equal(_raw(ovl["tensors"][r][k]), _raw(seq["tensors"][r][k])), (r, k)
        for l in range(2):
            for kind in ("weights", "wgrads"):
                assert np.array_equal(_raw(ovl[kind][r][l]["w"]), _raw(seq[kind][r][l]["w"])), (r, l, kind)
        assert kseq[r]["fp8"] == kovl[r]["fp8"] == 6 and kovl[r]["other_family"] == kovl[r]["no_form"] == 0, (kseq[r], kovl[r])
        assert koff[r] == dict.fromkeys(koff[r], 0) and not np.array_equal(_raw(off["tensors"][r][(1, "ah")]), _raw(ovl["tensors"][r][(1, "ah")]))


@pytest.mark.parametrize("F,options,moved_key", [(20, {"spmm_variant": 0}, "no_form"), (128, {"spmm_variant": 2, "spmm_blk_nb": 8}, "other_family")],
                         ids=["ld32", "k1s_takes_it"])
def test_not_taken_runs_as_with_the_mode_off_and_is_counted(da, F, options, moved_key):
    from helpers import make_ctx
    g = kr.graph203("real")
    N = kr.N_ROWS
    ctx = make_ctx(da, g, [F, F, 3], int(g["globalVtxCnt"]), options=options)
    rows = np.random.default_rng(101).uniform(-1, 1, (N + kr.N_SRC_GHOSTS, F)).astype(np.float32)
    off, _ = _aggregate(ctx, da, "fwd1", 0, rows, (N, F))
    k1s = ctx.get_option("spmm_launches_k1s")
    on, moved = _aggregate(ctx, da, "fwd1", 1, rows, (N, F))
    assert moved == dict(dict.fromkeys(moved, 0), **{moved_key: 1}), moved
    assert ctx.get_option("spmm_launches_k1s") - k1s == (1 if moved_key == "other_family" else 0)      # (K1s took it, not K1b)
    assert np.array_equal(_raw(on), _raw(off))
    ctx.close()


def test_refusals(da):
    from helpers import make_ctx
    g = kr.graph203("real")
    ctx = make_ctx(da, g, [8, 64], int(g["globalVtxCnt"]), gnn=da.GAT, options={"spmm_variant": 0})
    with pytest.raises(da.DoryError, match="DORY_GCN only"):
        ctx.k1_fp8_gather(1)
    ctx.k1_fp8_gather(0)
    ctx.close()
    ctx = make_ctx(da, g, [64, 64, 3], int(g["globalVtxCnt"]), options={"spmm_variant": 0, "gcn_bf16_gather": 1})
    assert ctx.k1_fp8_gather_stats() == dict.fromkeys(ctx.K1_FP8_GATHER_STATS, 0)      # the default is off
    with pytest.raises(da.DoryError, match="none of 0"):
        ctx.k1_fp8_gather(3)
    ctx.k1_fp8_gather(2)
    with pytest.raises(da.DoryError, match="one rounding"):
        ctx.aggregate(0, da.FORWARD)
    ctx.set_option("gcn_bf16_gather", 0)
    ctx.aggregate(0, da.FORWARD)
    ctx.labels_upload(np.zeros(kr.N_ROWS, np.uint32))
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    ctx.epoch_graph_begin()
    with pytest.raises(da.DoryError, match="recorded"):
        ctx.k1_fp8_gather(0)
    ctx.epoch_graph_end()
    ctx.close()


def test_training_on_the_golden_toy_graph_the_loss_falls(da):
    """twelve epochs on tests/golden/parts_toy60_p1 with mode 2 (rows of 64 floats in every aggregation): the loss of the last epoch's
    forward pass is under the first's"""
    import glob
    import os
    import partition_oracle as po
    d = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parts_toy60_p1")
    g = po.parse_graph_bin(open(glob.glob(os.path.join(d, "graph.*.bin"))[0], "rb").read())
    N, dims = int(g["localVtxCnt"]), [64, 64, 5]
    rng = np.random.default_rng(103)
    X = rng.uniform(-1, 1, (N, dims[0])).astype(np.float32)
    ctx = da.Context(0)
    ctx.configure(da.GCN, dims, N)
    ctx.set_option("spmm_variant", 0)
    ctx.graph_upload(g)
    ctx.preallocate()
    ctx.upload(0, "x", X)
    ctx.labels_upload((X @ rng.standard_normal((dims[0], dims[-1]))).argmax(axis=1).astype(np.uint32))
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    ctx.k1_fp8_gather(2)
    eng = da.NativeEngine(ctx)
    loss = []
    for _ in range(12):
        eng.run(1)
        loss.append(ctx.train_stat()[1])
    print("loss per epoch", loss)
    assert ctx.k1_fp8_gather_stats()["fp8"] == 36 and np.isfinite(loss).all() and loss[-1] < loss[0], loss
    eng.close()
    ctx.close()
