"""dory_gemm_bf16_send (include/dorylus_hip.h): with dory_halo_fused_pack on, a product dory_gemm_bf16's mode covers that feeds a halo
exchange runs a send form of K2b / K2c (csrc/gemm_bf16.hip, gemm_bf16_split.hip; the epilogue: gemm_bf16_tile.hpp) and the exchange runs
no pack kernel.  Every comparison is bit for bit: the product against the run with the fused pack off and the same bf16 mode, the bytes
on the wire against the pack kernel's, on the rigs of tests/test_gpu_halo_fused_pack.py and tests/test_gpu_halo_fused_pack_bf16.py."""
import numpy as np
import pytest

from test_gpu_halo_fused_pack import Rig, _bits, _golden, _random_parts, _same_bits
from test_gpu_halo_fused_pack_bf16 import Probe, _all_on

pytestmark = pytest.mark.gpu

# every form; M 1 / 129 / 300; cols 7 / 41 / 64 / 65 / 130 (both tile widths, a nearly empty second column tile, two workgroup columns);
# K 16 (less than one k-tile) / 130 (a ragged tail) / 602 (a split launch); xw = h W of a layer that narrows: K > cols
CASES = [(1, 7, 16, "h"), (129, 41, 130, "h"), (300, 130, 602, "h"), (129, 65, 602, "h"),
         (300, 64, 16, "z"), (129, 130, 130, "z"), (1, 65, 602, "z"),
         (129, 7, 16, "xw"), (300, 41, 602, "xw"), (129, 64, 130, "xw"),
         (300, 65, 16, "grad"), (1, 41, 130, "grad"), (129, 130, 602, "grad"), (300, 7, 130, "grad"), (129, 64, 602, "grad")]


@pytest.fixture(scope="module")
def da():
    import dorylus_amd
    return dorylus_amd


def _counters(ctx):
    g, s, x = ctx.gemm_bf16_stats(), ctx.gemm_bf16_send_stats(), ctx.gemm_bf16_split_stats()
    return np.array([s["send_launches"], s["plain_while_on"], g["bf16_launches"], g["fp32_while_on"], x["split_launches"]], np.int64)


@pytest.mark.parametrize("split", [0, 1], ids=["K2b", "K2c"])
@pytest.mark.parametrize("M,cols,K,form", CASES, ids=[f"M{m}-c{c}-K{k}-{f}" for m, c, k, f in CASES])
def test_send_epilogue_keeps_the_products_bits_and_writes_the_pack_kernels_bytes(da, M, cols, K, form, split):
    rig = Rig(da, M, cols, K, form)
    ctx, pr = rig.ctx, Probe(rig)
    ctx.gemm_bf16(1)
    ctx.gemm_bf16_split(split)
    rig.produce()                                                  # (a) the fused pack off, the bf16 mode on: the reference bits
    ref = _bits(ctx.download(*rig.src))
    n = ctx.gemm_bf16_stats()["bf16_launches"]                     # (the producer's NN / NT products: the one that travels, and for xw h@0 before it)
    assert n >= 1 and _counters(ctx).tolist() == [0, 0, n, 0, n * split]
    ctx.gemm_bf16_send(1)

    def fused_product(what):                                       # (b) the product under the fused pack: the bf16 send kernel ran
        before = _counters(ctx)
        rig.produce()
        assert (_counters(ctx) - before).tolist() == [1, 0, n, 0, n * split], (what, before, _counters(ctx))
        assert np.array_equal(_bits(ctx.download(*rig.src)), ref), (what, "the product's bits")
    ctx.halo_fused_pack(1)
    for exact in (0, 1):                                           # the fp32 wire, padded and exact-width rows
        ctx.set_option("halo_exact_rows", exact)
        fused_product(("fp32 wire", exact))
        rig.check_exchange((1, rig.total, 0), ("fp32 wire", exact))
    _all_on(rig)                                                   # the bf16 wire
    for exact in (1, 0):
        ctx.set_option("halo_exact_rows", exact)
        fused_product(("bf16 wire", exact))
        pr.check("fused16", ("bf16 wire", exact))
    if (M, cols, K, form) == (300, 130, 602, "h"):                 # (c) the switch off: the parent's launch, K2's fp32 send kernel
        ctx.gemm_bf16_send(0)
        before = _counters(ctx)
        rig.produce()
        assert (_counters(ctx) - before).tolist() == [0, 0, n - 1, 1, (n - 1) * split]
        assert not np.array_equal(_bits(ctx.download(*rig.src)), ref), "the fp32 kernel's bits: (b) did run the bf16 kernel"
        pr.check("fused16", "switch off")
    ctx.close()


def _epochs(da, make, split, fused, opts, downloads, dims=(20, 41, 6), epochs=3):
    """`epochs` GCN epochs over the in-process transport under gemm_bf16(1), K2b or K2c; fused: halo_fused_pack and the new switch on.
    Returns (run_local's result, {rank: (fused pack counters, fp32_while_on, send_launches)} read just before the contexts close)"""
    from local_ranks import run_local
    pobjs, parts = make()
    V, L = len(parts), len(dims) - 1
    rng = np.random.default_rng(5)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    labels = rng.integers(0, dims[-1], V).astype(np.uint32)
    Ws = [(rng.standard_normal((dims[i], dims[i + 1])) / np.sqrt(dims[i])).astype(np.float32) for i in range(L)]
    kept = {}

    def setup(ctx, r, g):
        if g["localVtxCnt"]:
            ctx.upload(0, "x", X[g["localToGlobal"]])
        if g["srcGhostCnt"]:
            ctx.upload(0, "fg", X[g["srcGhost"]].reshape(int(g["srcGhostCnt"]), dims[0]))
        ctx.labels_upload(labels[g["localToGlobal"]])
        for l, W in enumerate(Ws):
            ctx.weight_set(l, "w", W)
        assert bool(ctx.transform_first_layer(1)) == bool(opts.get("gcn_transform_first"))
        ctx.gemm_bf16(1)
        ctx.gemm_bf16_split(split)
        ctx.halo_fused_pack(fused)
        ctx.gemm_bf16_send(fused)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = (ctx.halo_fused_pack_stats(), ctx.gemm_bf16_stats()["fp32_while_on"], ctx.gemm_bf16_send_stats()["send_launches"])
            close()
        ctx.close = closing
    return run_local(da, pobjs, parts, list(dims), da.GCN, epochs, setup, dict(opts, spmm_blk_nb=8), downloads=downloads), kept


@pytest.mark.parametrize("split", [0, 1], ids=["K2b", "K2c"])
@pytest.mark.parametrize("case", ["parts_toy60_p2", "parts_toy40_p3_empty", "transform_first"])
def test_epochs_same_bits_and_every_gemm_exchange_fused(da, case, split):
    tf = case == "transform_first"
    make = _random_parts(da, 2) if tf else (lambda: _golden(da, case))          # (the golden partitions keep the aggregate-first order)
    dl = [(0, "z"), (1, "z"), (0, "h"), (0, "aTg")]
    dl += [(0, "ah"), (1, "xw"), (1, "fgxw")] if tf else [(0, "ah"), (1, "ah"), (1, "grad"), (1, "fg"), (0, "bg")]
    opts = {"gcn_transform_first": 2} if tf else {}
    off, k_off = _epochs(da, make, split, 0, opts, dl)
    on, k_on = _epochs(da, make, split, 1, opts, dl)
    _same_bits(off, on, (case, split, "fused pack off / on with dory_gemm_bf16_send"))
    for r, vw in enumerate(on["views"]):
        (fused, rows, fallback), fp32, sends = k_on[r]
        assert k_off[r] == ((0, 0, 0), 0, 0) and fp32 == 0, (case, r, k_off[r], k_on[r])
        if not int(vw["localVtxCnt"]):
            continue
        # aggregate-first: h@0 forward and grad@1 backward, both GEMM outputs; transform-first: xw@1 forward (g@1 backward: the tanh backward's)
        assert sends == fused == 3 * (1 if tf else 2) and (tf or fallback == 0), (case, r, k_on[r])
