#!/usr/bin/env python3
"""bench.py -- full-graph GCN epoch time + aggregated edges/s on a Reddit-scale
synthetic graph (BASELINE.json metric), on N MI355X of one node.

  python bench.py --gpus 1 --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
         --master-port P bench.py --gpus N --steps K --warmup W

A "step" is one synchronous training epoch of the reference's 2-layer GCN
(602-128-41) over the whole graph: 3 SpMMs (F = 602, 128, 128), 5 GEMMs, loss,
halo exchanges (N > 1), weight-gradient all-reduce (N > 1) and Adam -- nothing is
skipped or cached between epochs.  The graph (232 965 vertices, ~114.6 M directed
edges, symmetrised, self loops removed, seed 42) is partitioned in contiguous
blocks over the N ranks (strong scaling: the total work is fixed).  Inputs are
resident in HBM before the timed region.  One JSON line is printed by rank 0.

A plain run does only what the headline needs: setup, W warm-up steps, K timed steps and the line (ms_per_step = one
timed step).  --full adds everything else the line can carry: the CPU baseline, the transform-first and cached-ah0
epochs and the other single-GPU configurations.  --dump-outputs DIR writes what the last timed step computed as
DIR/<name>.npy (dump_outputs); the inputs are seeded, so two builds run with the same arguments compare output for output.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
# What the 1e-4 parity criterion does NOT rest on reference-generated numbers for: these pieces are
# checked against a restatement of the reference's source only -- its own build needs cblas / boost headers the image
# lacks -- and the 8-head GAT has no reference implementation at all.  Pinned: partition / CSC / CSR indexing (bytes the
# reference's DataLoader wrote), GCN aggregate + GEMM + tanh + softmax-label + dW (the reference's numpy-gnn), Adam step 1.
PARITY_UNPINNED = ["gat edge ops (CPU_comm.cpp:161-242,299-408)", "maskout / val-stat (CPU_comm.cpp:464-471)",
                   "adam beyond step 1 (AdamOptimizer.cpp:29-51)", "xavier stream (weightserver.cpp:567-585)",
                   "gatmh (8-head softmax GAT: no reference implementation)"]
sys.path.insert(0, ROOT)

REDDIT_V = 232965
REDDIT_E = 114615892
DIMS = [602, 128, 41]          # run/reddit.config
# other BASELINE.json configs (parity/scale cases, not the headline line): SURVEY.md 8(d) shapes
WORKLOADS = {
    "reddit": (REDDIT_V, REDDIT_E, [602, 128, 41]),
    "amazon": (9430088, 231594310, [300, 64, 64, 25]),          # config 4: Amazon GCN 3-layer
    "friendster": (65608366, 3612134270, [256, 48, 51]),        # config 5 (use --emulate r/8: one rank's partition)
}


def synth_edges(kind, V, E, seed=42):
    """seeded symmetric edge records (src, dst); self loops are dropped by the builder
    (dataloader.cpp:268-269) exactly as the reference does."""
    rng = np.random.default_rng(seed)
    half = E // 2
    if kind == "uniform":
        s = rng.integers(0, V, half, dtype=np.uint32)
        d = rng.integers(0, V, half, dtype=np.uint32)
    elif kind == "powerlaw":
        # skewed endpoints: id ~ V * u^1.5 (ids shuffled) puts ~2.6e-4 of all endpoints on the
        # top vertex -> max degree ~3e4 at Reddit scale, the order of real Reddit's 21 657
        perm = rng.permutation(V).astype(np.uint32)
        s = perm[np.minimum((rng.random(half) ** 1.5 * V).astype(np.int64), V - 1)]
        d = perm[np.minimum((rng.random(half) ** 1.5 * V).astype(np.int64), V - 1)]
    elif kind == "rmat":
        # R-MAT, a=.57 b=.19 c=.19 d=.05, ceil(log2 V) levels (18 at Reddit scale; ids folded back with
        # mod V), ids shuffled.  Far more skewed than real Reddit: the top vertices carry ~1 % of all endpoints each.
        levels = max(1, int(np.ceil(np.log2(V))))
        s = np.zeros(half, np.uint32)
        d = np.zeros(half, np.uint32)
        for _ in range(levels):
            r = rng.random(half, dtype=np.float32)
            sb = (r >= 0.76).astype(np.uint32)                       # quadrants c, d: source bit 1
            db = (((r >= 0.57) & (r < 0.76)) | (r >= 0.95)).astype(np.uint32)   # quadrants b, d: destination bit 1
            s = (s << np.uint32(1)) | sb
            d = (d << np.uint32(1)) | db
        perm = rng.permutation(V).astype(np.uint32)
        s, d = perm[s % np.uint32(V)], perm[d % np.uint32(V)]
    elif kind == "hub":
        # uniform, plus one vertex that is an endpoint of 1 % of all edges (degree ~1.1 M: 50x real Reddit's maximum):
        # the stress case for anything that walks a row's edge list on one lane group
        s = rng.integers(0, V, half, dtype=np.uint32)
        d = rng.integers(0, V, half, dtype=np.uint32)
        d[rng.random(half) < 0.01] = 12345
    elif kind == "community":
        # 50 equal communities of consecutive ids (what a METIS-ordered Reddit looks like to the
        # kernels: subreddits): 85 % of the edges stay inside the source's community
        C = 50
        s = rng.integers(0, V, half, dtype=np.uint32)
        size = (V + C - 1) // C
        inside = rng.random(half) < 0.85
        local = (s // size).astype(np.int64) * size + rng.integers(0, size, half)
        d = np.where(inside, np.minimum(local, V - 1), rng.integers(0, V, half)).astype(np.uint32)
    else:
        raise ValueError(kind)
    return np.concatenate([s, d]), np.concatenate([d, s])


def block_bounds(V, pw, r):
    """contiguous vertex blocks: vertex v belongs to rank v * pw // V"""
    return -(-r * V // pw), -(-(r + 1) * V // pw)


def synth_incident_edges(V, E, pr, pw, seed=42):
    """The records of a uniform synthetic graph of ~E directed edges that are incident to rank pr's contiguous block --
    all a rank needs (a record matters to a rank iff its source or its destination is local; the reference's DataLoader
    skips the others, dataloader.cpp:268-297), without the whole record list in host memory (Friendster: 29 GB).  The
    undirected pairs between block i and block j come from a generator seeded by the UNORDERED pair {i, j}, so the ranks of
    a real N-GPU run generate the same pair set for the edges they share: the partitions are those of ONE global graph.
    Expected pairs: E/2 x 2/pw^2 between two different blocks, E/2 / pw^2 inside a block."""
    lo, hi = block_bounds(V, pw, pr)
    half = E // 2
    srcs, dsts = [], []
    for j in range(pw):
        i0, j0 = min(pr, j), max(pr, j)
        m = half // (pw * pw) if j == pr else 2 * half // (pw * pw)
        rng = np.random.default_rng([seed, i0, j0])
        lo_i, hi_i = block_bounds(V, pw, i0)
        lo_j, hi_j = block_bounds(V, pw, j0)
        a_ = rng.integers(lo_i, hi_i, m, dtype=np.uint32)      # endpoint in block i0
        b_ = rng.integers(lo_j, hi_j, m, dtype=np.uint32)      # endpoint in block j0
        srcs += [a_, b_]
        dsts += [b_, a_]
    return np.concatenate(srcs), np.concatenate(dsts)


def splitmix_uniform(seed, rows_global, cols, lo=-1.0, hi=1.0):
    """host twin of the device counter RNG (csrc/elementwise.hip fill_uniform_kernel)"""
    rows_global = np.asarray(rows_global, dtype=np.uint64)
    idx = rows_global[:, None] * np.uint64(cols) + np.arange(cols, dtype=np.uint64)[None, :]
    with np.errstate(over="ignore"):
        x = (np.uint64(seed) ^ idx) + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        x = x ^ (x >> np.uint64(31))
    u = (x >> np.uint64(40)).astype(np.float32) * np.float32(1.0 / 16777216.0)
    return (np.float32(lo) + (np.float32(hi) - np.float32(lo)) * u).astype(np.float32)


def halo_selfcheck(ctx, g, da):
    """N > 1 only, before any timing: one forward and one backward halo exchange of rows
    that are a known function of the global vertex id; every received ghost row must be
    the owner's row bit for bit (plan + pack + RCCL all-to-all-v + unpack end to end).
    Then the overlapped schedule (local-source blocks of the SpMM running under the
    exchange) must give bit-identical aggregates to the sequential one."""
    ctx.fill_uniform(0, "h", 7, -1.0, 1.0, g["localToGlobal"])
    ctx.halo_exchange(1, da.FORWARD)
    ctx.sync()
    ok = np.array_equal(ctx.download(1, "fg"), splitmix_uniform(7, g["srcGhost"], DIMS[1]))
    ctx.fill_uniform(1, "grad", 9, -1.0, 1.0, g["localToGlobal"])
    ctx.halo_exchange(1, da.BACKWARD)
    ctx.sync()
    ok = ok and np.array_equal(ctx.download(0, "bg"), splitmix_uniform(9, g["dstGhost"], DIMS[1]))
    res = {}
    for overlap in (0, 1):
        ctx.set_option("halo_overlap", overlap)
        ctx.fill_uniform(0, "h", 7, -1.0, 1.0, g["localToGlobal"])
        ctx.halo_exchange(1, da.FORWARD)
        ctx.aggregate(1, da.FORWARD)          # consumes fg@1: split launch when overlap is on
        ctx.halo_exchange(1, da.BACKWARD)
        ctx.aggregate(1, da.BACKWARD)
        ctx.sync()
        res[overlap] = (ctx.download(1, "ah"), ctx.download(0, "aTg"))
    ok = ok and np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    return bool(ok)


def halo_selfcheck_gat(ctx, g, da, gnn):
    """the same for the GAT orders (Engine::scatterGAT / ghostReceiverGAT, gat_ops.cpp:277-435): `z` travels forward into
    fg_z, `grad` backward into bg_d (the multi-head extension ships dO and its statistics inside its backward aggregate,
    so only its forward exchange is checked here); every received row must be the owner's row bit for bit."""
    ctx.fill_uniform(0, "z", 7, -1.0, 1.0, g["localToGlobal"])
    ctx.halo_exchange(1, da.FORWARD)
    ctx.sync()
    zc = ctx.info(0, "z")[1]
    ok = np.array_equal(ctx.download(0, "fg_z"), splitmix_uniform(7, g["srcGhost"], zc))
    if gnn == "gat":
        ctx.fill_uniform(0, "grad", 9, -1.0, 1.0, g["localToGlobal"])
        ctx.halo_exchange(1, da.BACKWARD)
        ctx.sync()
        ok = ok and np.array_equal(ctx.download(0, "bg_d"), splitmix_uniform(9, g["dstGhost"], ctx.info(0, "grad")[1]))
    return bool(ok)


def git_blob_sha1(path):
    """what `git hash-object` prints (the GPU box has no .git): sha1("blob <len>\\0" + content)"""
    import hashlib
    data = open(path, "rb").read()
    return hashlib.sha1(b"blob %d\0" % len(data) + data).hexdigest()


def spmm_source_stamp():
    """what a PMC traffic figure is stamped with: the CODE of the aggregation kernels (K1 / K1s in spmm.hip, the sweep
    skeleton they run on in sweep_core.hpp since round 5) -- one hash over both files with comments and white space removed,
    so that a reworded comment does not orphan a measurement while any change the compiler sees does"""
    import hashlib
    import re
    d = os.path.join(ROOT, "dorylus_amd", "csrc")
    h = hashlib.sha1()
    for f in ("spmm.hip", "sweep_core.hpp"):
        with open(os.path.join(d, f), "r", encoding="utf-8") as fh:
            src = fh.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)      # block comments
        src = re.sub(r"//[^\n]*", " ", src)                   # line comments (no string literal in these files holds "//")
        h.update(re.sub(r"\s+", " ", src).encode())
    return h.hexdigest()


def source_stamp(files):
    """as spmm_source_stamp, over any set of kernel sources (comments and white space removed)"""
    import hashlib
    import re
    d = os.path.join(ROOT, "dorylus_amd", "csrc")
    h = hashlib.sha1()
    for f in files:
        with open(os.path.join(d, f), "r", encoding="utf-8") as fh:
            src = fh.read()
        src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
        src = re.sub(r"//[^\n]*", " ", src)
        h.update(re.sub(r"\s+", " ", src).encode())
    return h.hexdigest()


GATMH_STAMP_FILES = ("gat_mh_sweep.hip", "sweep_core.hpp")


def spmm_algorithmic_bytes(N, G, E, F):
    """compulsory bytes of one SpMM launch."""
    return E * 8 + 8 * (N + 1) + 4 * N + 4 * F * (N + G) + 4 * F * N


DUMP_WEIGHTS = {"gcn": ("w",), "gat": ("w", "a_i"), "gatmh": ("w", "a_l", "a_r")}
DUMP_ROW_BYTES = 48 << 20      # budget of the row-sampled activations; weights and statistics are a few MB at most


def dump_outputs(ctx, g, gnn, out_dir):
    """--dump-outputs: what one timed epoch hands its caller, read back after the last one.  Every layer's weights after its
    Adam step (W<l>, plus a_i<l> / a_l<l> / a_r<l> for the GAT forms) and their gradients (dW<l>, ...), the training
    statistics (train_stat: accuracy sum, loss sum, validation rows) and the activations the epoch leaves behind: hidden
    outputs h<l> and the last layer's logits.  Activations are row-sampled: a fixed seeded subset of the local rows, the same
    for every tensor and every run with the same arguments, within DUMP_ROW_BYTES; rows.npy holds their global vertex ids.
    float32 as computed, except rows and train_stat (float64)."""
    os.makedirs(out_dir, exist_ok=True)
    L = ctx.L
    out = {}
    for l in range(L):
        for name in DUMP_WEIGHTS[gnn]:
            tag = "W" if name == "w" else name
            out[f"{tag}{l}"] = ctx.weight_get(l, name)
            out[f"d{tag}{l}"] = ctx.weight_grad_get(l, name)
    a, lo, n = ctx.train_stat()
    out["train_stat"] = np.array([a, lo, n], np.float64)
    if gnn == "gcn":
        acts = [(f"h{l}", l, "h") for l in range(L - 1)] + [("logits", L - 1, "z")]
    else:
        acts = [(f"h{l}", l, "h") for l in range(1, L)] + [("logits", L - 1, "ah" if gnn == "gat" else "logits")]
    N = int(g["localVtxCnt"])
    cols = sum(ctx.info(l, t)[1] for _, l, t in acts)
    k = min(N, max(1, DUMP_ROW_BYTES // (4 * cols)))
    rows = np.arange(N) if k == N else np.sort(np.random.default_rng(0).choice(N, k, replace=False))
    out["rows"] = np.asarray(g["localToGlobal"])[rows].astype(np.float64)
    for key, l, t in acts:
        out[key] = np.ascontiguousarray(ctx.download(l, t)[rows])
    for key, arr in out.items():
        np.save(os.path.join(out_dir, key + ".npy"), arr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--graph", default="uniform", choices=["uniform", "powerlaw", "rmat", "community", "hub"])
    ap.add_argument("--scale", type=float, default=1.0, help="edge-count scale (1.0 = Reddit)")
    ap.add_argument("--workload", default="reddit", choices=sorted(WORKLOADS),
                    help="graph/model shape; anything but reddit is a scale test, not the BASELINE metric line")
    ap.add_argument("--gnn", default="gcn", choices=["gcn", "gat", "gatmh"],
                    help="gat = the reference's GAT prototype (BASELINE config 3's weighted-SpMM part); gatmh = the "
                         "8-head per-edge-softmax extension (config 3's wording; no reference oracle); not the headline metric")
    ap.add_argument("--emulate", default="", help="R/P: run rank R's partition of a P-way split alone on one GPU, "
                    "halo exchange skipped (per-rank compute time of an N-GPU run; diagnostic, not the metric)")
    ap.add_argument("--opt", nargs="*", default=[], help="context options key=value (diagnostic runs, e.g. spmm_variant=0)")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--no-alt", action="store_true", help="skip the extra transform-first epochs (profiling runs: only the headline kernels)")
    ap.add_argument("--cpu-rows", type=int, default=0, help="restrict the CPU baseline to the first rows (0 = the full epoch)")
    ap.add_argument("--transport", default="rccl", choices=["rccl", "host"],
                    help="rccl = the product path (grouped ncclSend/ncclRecv + ncclAllReduce over xGMI).  host = dry run of the "
                         "N > 1 logic where RCCL cannot run: the packed rows and the gradients travel through "
                         "dory_comm_set_host_transport over gloo (several ranks on ONE GPU: --device 0); diagnostic, not the metric")
    ap.add_argument("--device", type=int, default=-1, help="HIP device of this rank (default: LOCAL_RANK)")
    ap.add_argument("--with-friendster", action="store_true",
                    help="with --full: also time BASELINE config 5 as rank 0 of 8 holds it (key friendster_rank0of8: ~2 min of setup, "
                         "58 GB of ghost rows)")
    ap.add_argument("--full", action="store_true",
                    help="also run what the headline does not need: the CPU baseline, the transform-first and cached-ah0 epochs and "
                         "the other single-GPU configurations (gat, gatmh, rmat, community, amazon_rank0of8); without it their keys "
                         "are null or absent")
    ap.add_argument("--dump-outputs", metavar="DIR", default="",
                    help="after the timed steps, write what the last one computed (weights, weight gradients, training statistics, "
                         "a fixed seeded row sample of the hidden and output activations) as DIR/<name>.npy")
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")

    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    if world != args.gpus:
        if world == 1 and args.gpus > 1:
            raise SystemExit("launch with torch.distributed.run for --gpus > 1")
        args.gpus = world

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL across processes needs it on this driver
    import torch
    import torch.distributed as dist
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU (there is no CPU fallback for the product path)")
    dev = args.device if args.device >= 0 else local_rank
    host_tx = args.transport == "host"
    tdev = "cpu" if host_tx else "cuda"     # where the few scalars torch.distributed reduces live (gloo: host)
    torch.cuda.set_device(dev)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        # (RCCL's exchange kernels run beside the local-source K1s launch and take CUs from it; no channel cap is set here --
        #  the warm-up samples spmm_sweep_reserve_cus instead, below -- and whatever NCCL_* the caller exported is reported)
        with stdout_to_stderr():
            if host_tx:
                dist.init_process_group(backend="gloo")
            else:
                dist.init_process_group(backend="nccl", device_id=torch.device("cuda", dev))
            dist.barrier()          # creates torch's communicator now, not inside the timed region
    import dorylus_amd as da

    preflight = None
    if world > 1:
        preflight = first_contact_preflight(da, dist, torch, rank, world, dev, host_tx, tdev)
        # a hang inside the epochs of a first multi-GPU run (an exchange that never completes) must end with a message
        # that says where, not with the driver's own kill: whole-run watchdog, generous against the ~1 min a run takes
        import threading
        run_stage = {"name": "setup (graph generation, partition build, upload)"}

        def run_watchdog(limit=float(os.environ.get("DORY_BENCH_WATCHDOG_S", "1500"))):
            time.sleep(limit)
            sys.stderr.write("bench.py: rank %d still running after %.0f s, last stage: %s -- giving up\n" % (rank, limit, run_stage["name"]))
            sys.stderr.flush()
            os._exit(4)
        threading.Thread(target=run_watchdog, daemon=True).start()
    else:
        run_stage = {"name": ""}

    global DIMS
    V, E_full, DIMS = WORKLOADS[args.workload]
    E_target = int(E_full * args.scale)
    t_setup = time.time()
    pw, pr = world, rank
    if args.emulate:
        pr, pw = (int(t) for t in args.emulate.split("/"))
    if args.workload in ("friendster", "amazon") and args.graph == "uniform" and pw > 1:
        # configs 4 and 5 as a rank holds them (one rank emulated, or a real N-GPU run): only the records incident to
        # the rank's block, generated consistently across ranks (tests/test_gpu_fullscale.py does the same)
        src, dst = synth_incident_edges(V, E_target, pr, pw)
    else:
        src, dst = synth_edges(args.graph, V, E_target)
    parts = (np.arange(V, dtype=np.int64) * pw // V).astype(np.int32)   # contiguous blocks
    if world > 1:   # every rank builds its own partition at the same time: share the host cores
        os.environ.setdefault("DORY_BUILD_THREADS", str(max(1, min(32, usable_cpus() // world))))
    part = da.Partition.build(src, dst, parts, pr, pw)
    del src, dst
    g = part.view()
    N, Gs, Gd = int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
    nnz_in, nnz_out = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])

    ctx = da.Context(dev)
    gat = args.gnn in ("gat", "gatmh")
    ctx.configure({"gcn": da.GCN, "gat": da.GAT, "gatmh": da.GATMH}[args.gnn], DIMS, V, rank, world)
    if args.gnn == "gatmh":
        ctx.gatmh_heads([8, 1])
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    part.upload(ctx, parts if world > 1 else None)
    ctx.preallocate()
    # synthetic features: fp32 U(-1,1) keyed by global vertex id (same row whichever rank
    # holds it); layer-0 ghost rows are "loaded from file" once, like fg@0 in the reference
    ctx.fill_uniform(0, "h" if gat else "x", 1, -1.0, 1.0, g["localToGlobal"])
    if Gs and not gat:
        ctx.fill_uniform(0, "fg", 1, -1.0, 1.0, g["srcGhost"])
    labels = np.random.default_rng(2).integers(0, DIMS[-1], V).astype(np.uint32)
    ctx.labels_upload(labels[g["localToGlobal"]])
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    if world > 1 and host_tx:
        set_gloo_transport(ctx, dist, torch, rank, world)
    elif world > 1:
        idt = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            idt.copy_(torch.from_numpy(ctx.comm_unique_id()))
        with stdout_to_stderr():
            dist.broadcast(idt, 0)
            ctx.comm_init(idt.cpu().numpy(), rank, world)
    halo_ok = None
    run_stage["name"] = "halo self-check (two exchanges + overlapped / sequential aggregates)"
    if world > 1:
        flag = torch.tensor([1 if (halo_selfcheck_gat(ctx, g, da, args.gnn) if gat else halo_selfcheck(ctx, g, da)) else 0], dtype=torch.int32, device=tdev)
        dist.all_reduce(flag, op=dist.ReduceOp.MIN)
        halo_ok = bool(flag.item())
        if not halo_ok:
            raise SystemExit("halo exchange self-check FAILED: received ghost rows differ from the owners' rows")
    eng = da.NativeEngine(ctx)
    t_setup = time.time() - t_setup

    def barrier():
        ctx.sync()
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()

    # ---- N > 1: how many CUs do the exchange's kernels really take beside K1s?  Three extra warm-up epochs, one per
    # candidate reserve, smallest first; a reserve holds if no rank counted a gate timeout in its epoch ----
    reserve_probe = None
    run_stage["name"] = "reserve probe (one epoch per candidate spmm_sweep_reserve_cus)"
    if world > 1 and not gat and ctx.get_option("spmm_variant") == 2 and not any(o.startswith("spmm_sweep_reserve_cus=") for o in args.opt):
        reserve_probe = {"tried": [], "chosen": None}
        for cand in (2, 4, 8):
            ctx.set_option("spmm_sweep_reserve_cus", cand)
            ctx.set_option("spmm_gates_rearm", 1)            # a timeout of the previous candidate must not hide this one's
            before = ctx.get_option("spmm_gate_timeouts")
            eng.run(1)
            d_ = torch.tensor([ctx.get_option("spmm_gate_timeouts") - before], dtype=torch.int64, device=tdev)
            dist.all_reduce(d_, op=dist.ReduceOp.MAX)
            reserve_probe["tried"].append({"reserve_cus": cand, "gate_timeouts_max_rank": int(d_.item())})
            if int(d_.item()) == 0:
                reserve_probe["chosen"] = cand
                break
        if reserve_probe["chosen"] is None:                 # even 8 CUs per XCD were not enough: keep 8, the counters below say so
            reserve_probe["chosen"] = 8
        ctx.set_option("spmm_sweep_reserve_cus", reserve_probe["chosen"])
        ctx.set_option("spmm_gates_rearm", 1)

    # ---- warmup, then exactly K timed steps ------------------------------------------
    run_stage["name"] = "warm-up + timed epochs"
    if args.warmup:
        eng.run(args.warmup)
    ctx.timing_reset()
    ctx.timing_enable(True)        # HIP events on the kernels' own stream, over the timed region
    barrier()
    t0 = time.perf_counter()
    epoch_ms = eng.run(args.steps)
    barrier()
    elapsed = time.perf_counter() - t0
    if world > 1:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=tdev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
        cnt = torch.tensor([nnz_in, nnz_out], dtype=torch.int64, device=tdev)
        dist.all_reduce(cnt)
        E_in, E_out = int(cnt[0]), int(cnt[1])
    else:
        E_in, E_out = nnz_in, nnz_out
    ms_per_step = elapsed * 1e3 / args.steps
    if args.dump_outputs and rank == 0:
        run_stage["name"] = "writing the last timed step's outputs"
        dump_outputs(ctx, g, args.gnn, args.dump_outputs)
    run_stage["name"] = "bookkeeping after the timed region"
    nl = len(DIMS) - 1
    edges_per_epoch = nl * E_in + (nl - 1) * E_out           # L forward (CSC) + L-1 backward (CSR) aggregations
    tf_mode = (not gat) and ctx.transform_first_active()          # diagnostic: A(XW0) order, one more d1-wide CSR pass for dW0
    if tf_mode:
        edges_per_epoch = nl * E_in + nl * E_out
    if gat:                                                  # 2 fwd (CSC) + 2 bwd x (CSR + CSC) aggregations
        edges_per_epoch = 4 * E_in + 2 * E_out               # (gatmh: the count of round 1-4's six passes is kept so that edges/s stays comparable)
    value = edges_per_epoch / (ms_per_step * 1e-3)

    # ---- roofline of the dominant kernel (K1 SpMM): HIP events recorded during the timed steps ----
    fam = {}
    for f in ("spmm", "gemm", "loss", "halo", "allreduce", "adam", "halo_deferred", "halo_hidden", "spmm_beside_halo"):
        ms, n = ctx.timing_get(f)
        fam[f] = (ms, n)
    ctx.timing_enable(False)
    spmm_ms, spmm_n = fam["spmm"]
    algo = (spmm_algorithmic_bytes(N, Gs, nnz_in, DIMS[0]) + spmm_algorithmic_bytes(N, Gs, nnz_in, DIMS[1]) +
            spmm_algorithmic_bytes(N, Gd, nnz_out, DIMS[1]))  # bytes of the 3 launches of one epoch
    launches_per_epoch = 3
    avg_launch_ms = spmm_ms / max(spmm_n, 1)
    achieved = (algo / launches_per_epoch) / (avg_launch_ms * 1e-3) / 1e9   # GB/s per average launch
    variant = ctx.get_option("spmm_variant")
    kernel_name = {2: "spmm_sweep_kernel<32,R,false,PAIR> (K1s: register accumulators, gated per-XCD sweep over the source blocks; one aggregate = one launch)",
                   1: "spmm_blocked_kernel<32> + spmm_reduce_kernel (K1b; one aggregate = both)",
                   0: "spmm_rows_kernel<64,3> / <32,1> (K1 row gather)"}.get(variant, "spmm")
    traffic = None   # HBM-side bytes per launch: separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of this same command (profiles/)
    traffic_src = None
    try:
        pm = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json")))
        if world == 1 and args.graph == "uniform" and args.scale == 1.0 and not args.emulate and args.workload == "reddit" and not args.opt:
            ent = pm["spmm_variant_%d" % variant]
            # the counters were collected for ONE version of the kernel source: a later edit of spmm.hip without a new
            # collection must not leave a stale number in the record
            have = spmm_source_stamp()
            if ent.get("spmm_hip_blob") in (None, have) or variant != 2:
                traffic = ent["bytes_per_launch"]
                traffic_src = ent.get("source")
                if variant == 2 and ent.get("spmm_hip_blob") is None:
                    traffic_src = (traffic_src or []) + ["(entry carries no spmm.hip blob hash: collected before round 3)"]
            else:
                traffic_src = ["stale: profiles/pmc_traffic.json was collected for spmm.hip blob %s, this build is %s -- "
                               "re-run tools/collect_profiles.sh" % (ent.get("spmm_hip_blob"), have)]
    except (OSError, KeyError, ValueError):
        pass
    roofline = {"bound": "hbm", "achieved": round(achieved, 2), "peak": 8000.0, "unit": "GB/s",
                "frac": round(achieved / 8000.0, 5), "traffic": traffic, "traffic_source": traffic_src,
                "kernel": kernel_name, "avg_launch_ms": round(avg_launch_ms, 4),
                "algorithmic_bytes_per_launch": int(algo / launches_per_epoch),
                "gather_bytes_per_launch": int((nnz_in * 608 + nnz_in * 128 + nnz_out * 128) * 4 / 3),
                "l2_gather_TBps": round((nnz_in * 608 + nnz_in * 128 + nnz_out * 128) * 4 / 3 / (avg_launch_ms * 1e-3) / 1e12, 2)}
    # the ceiling that actually binds the gather: every edge moves one row slab L2 -> L1 -> registers, and a CU's vector
    # memory path delivers 64 B per clock: 64 B x 256 CUs x 2.3 GHz = 37.7 TB/s (the HBM fraction above stays the headline)
    roofline["l1_path"] = {"peak_TBps": 37.7, "achieved_TBps": roofline["l2_gather_TBps"],
                           "frac": round(roofline["l2_gather_TBps"] / 37.7, 4),
                           "frac_of_guide_l2_34.5_TBps": round(roofline["l2_gather_TBps"] / 34.5, 4),
                           "frac_of_measured_gather_ceiling_31_TBps": round(roofline["l2_gather_TBps"] / 31.0, 4),
                           "what": "gathered row bytes (E x ld x 4 per launch) / launch time against (a) 64 B/clk/CU x 256 CUs x 2.3 GHz, "
                                   "(b) MI355X_MICROARCH.md's aggregate L2 figure, (c) what a pure L2-resident gather reaches on this "
                                   "chip (tools/probes/gather_probe.hip, profiles/r02_gather_probe_l2_ceiling.txt: 30-32 TB/s)"}

    # second kernel family: the dense transforms on fp32 MFMA (all GEMMs of the epoch, split-K stages included)
    gemm_ms, gemm_n = fam["gemm"]
    d0, d1, d2 = (list(DIMS) + [0, 0, 0])[:3]
    gemm_flops = 2.0 * N * (2 * d0 * d1 + 3 * d1 * d2) if len(DIMS) == 3 else 0.0   # z0, dW0 | z1, grad1, dW1
    roofline_gemm = None
    if gemm_ms > 0 and gemm_flops:
        tf = gemm_flops * args.steps / (gemm_ms * 1e-3) / 1e12
        roofline_gemm = {"bound": "mfma", "achieved": round(tf, 2), "peak": 157.0, "unit": "TFLOP/s",
                         "frac": round(tf / 157.0, 4), "kernel": "gemm_dma_kernel<BN,...> fp32 MFMA 32x32x2, operand tiles by LDS-DMA (+ split-K reduce)",
                         "flops_per_epoch": int(gemm_flops), "ms_per_epoch": round(gemm_ms / args.steps, 4)}

    # ---- CPU baseline: the oracle (port of the reference CPU path) on this box's cores ----------
    cpu = None
    if args.full and rank == 0 and world == 1 and not args.no_cpu_baseline and not gat and not args.emulate and args.workload == "reddit":
        cpu = cpu_baseline(ctx, g, args.cpu_rows)

    # ---- the same epoch in the transform-first order of layer 0 (opt-in mode, reported beside the headline) ----
    alt = None
    if args.full and world == 1 and not gat and not tf_mode and not args.emulate and not args.opt and not args.no_alt:
        ctx.set_option("gcn_transform_first", 2)
        if ctx.transform_first_active():
            ctx.timing_enable(False)
            eng.run(max(1, args.warmup))
            alt_ms = eng.run(args.steps)
            nar = [l for l in range(nl) if ctx.transform_first_layer(l)]
            alt = {"order": "transform-first on layers %s [opt-in gcn_transform_first=2: z_l = A(in_l W_l), dW_l = in_l^T(A^T g_l); "
                            "not the reference order]" % nar,
                   "ms_per_step": float(np.mean(alt_ms)), "epoch_ms_median": float(np.median(alt_ms)),
                   "aggregation_widths": [DIMS[l + 1] if l in nar else DIMS[l] for l in range(nl)]}
        ctx.set_option("gcn_transform_first", 0)

    # ---- the same epoch with the layer-0 aggregate kept across epochs (opt-in gcn_cache_ah0, reported beside the headline) ----
    cached = None
    if args.full and world == 1 and not gat and not tf_mode and not args.emulate and not args.opt and not args.no_alt:
        ctx.set_option("gcn_cache_ah0", 1)
        ctx.timing_enable(False)
        eng.run(max(1, args.warmup))          # (computes ah@0 once)
        ctx.sync()
        t1 = time.perf_counter()
        c_ms = eng.run(args.steps)
        ctx.sync()
        c_ms_per = (time.perf_counter() - t1) * 1e3 / args.steps
        e_cached = (nl - 1) * E_in + (nl - 1) * E_out     # the layer-0 aggregation is not executed: 2 E per epoch, not 3 E
        cached = {"what": "opt-in gcn_cache_ah0=1: ah@0 = A_hat x is a constant of full-graph training (x, fg@0 and the adjacency "
                          "never change) and stays resident; every other stage as in the headline; not the reference's schedule",
                  "ms_per_step": c_ms_per, "epoch_ms_median": float(np.median(c_ms)),
                  "edges_per_epoch": int(e_cached), "edges_per_s": e_cached / (c_ms_per * 1e-3),
                  "aggregations_skipped": int(ctx.get_option("gcn_cache_ah0_skips"))}
        ctx.set_option("gcn_cache_ah0", 0)
    gates = {"timeouts": int(ctx.get_option("spmm_gate_timeouts")), "ungated_launches": int(ctx.get_option("spmm_ungated_launches")),
             "spmm_sweep_reserve_cus": int(ctx.get_option("spmm_sweep_reserve_cus")),
             # K1s's placement assumption (workgroup id & 7 = XCD, eight XCDs), checked once per context at dory_create; when it
             # fails the gated / ungated form is chosen by measurement (policy 0 / 8; -1 = nothing to decide)
             "xcd_mapping_ok": bool(ctx.get_option("spmm_xcd_mapping_ok")), "xcd_count": int(ctx.get_option("spmm_xcd_count")),
             "xcd_policy": int(ctx.get_option("spmm_xcd_policy")),
             "note": "K1s sweeps whose workgroups were not co-resident within the polling bound (then the launch and the next 16 "
                     "ran ungated: same results, unsynchronised rate); 0 / 0 is the healthy state"}

    # ---- multi-GPU bookkeeping: load balance, halo volume, link rate ----
    multi = None
    if world > 1:
        ld1 = (DIMS[1] + 31) // 32 * 32
        mine = torch.tensor([nnz_in, N, Gs * ld1 * 4 + Gd * ld1 * 4, fam["halo"][0], fam["allreduce"][0],
                             gates["timeouts"], gates["ungated_launches"], fam["halo_deferred"][0], fam["halo_hidden"][0],
                             fam["spmm_beside_halo"][0]], dtype=torch.float64, device=tdev)
        allr = [torch.zeros_like(mine) for _ in range(world)]
        dist.all_gather(allr, mine)
        A = np.array([t.cpu().numpy() for t in allr])
        halo_ms = A[:, 3] / args.steps
        multi = {"nnz_in_per_rank_max": int(A[:, 0].max()), "nnz_in_per_rank_mean": float(A[:, 0].mean()),
                 "nnz_max_over_mean": float(A[:, 0].max() / max(A[:, 0].mean(), 1.0)),
                 "vertices_per_rank": [int(v) for v in A[:, 1]],
                 "halo_bytes_received_per_epoch_total": int(A[:, 2].sum()),
                 "halo_bytes_received_per_epoch_max_rank": int(A[:, 2].max()),
                 "halo_ms_per_epoch_max_rank": float(halo_ms.max()),
                 "halo_GBps_per_rank_min": float((A[:, 2] / np.maximum(halo_ms, 1e-9) / 1e6).min()),
                 "allreduce_ms_per_epoch_max_rank": float((A[:, 4] / args.steps).max()),
                 "spmm_gate_timeouts_per_rank": [int(v) for v in A[:, 5]], "spmm_ungated_launches_per_rank": [int(v) for v in A[:, 6]],
                 "halo_overlap": int(ctx.get_option("halo_overlap")), "spmm_sweep_reserve_cus": gates["spmm_sweep_reserve_cus"],
                 # exchange time hidden under the local-source launch / exchange time, per rank (HIP events of both streams on
                 # the device clock; exchanges the compute stream waited for at once are not in the denominator)
                 "halo_overlap_fraction_per_rank": [round(float(h / d), 4) if d > 0 else None for h, d in zip(A[:, 8], A[:, 7])],
                 "halo_overlap_fraction_min": (float(np.min([h / d for h, d in zip(A[:, 8], A[:, 7]) if d > 0])) if (A[:, 7] > 0).any() else None),
                 "halo_deferred_ms_per_epoch_max_rank": float((A[:, 7] / args.steps).max()),
                 "spmm_beside_halo_ms_per_epoch_max_rank": float((A[:, 9] / args.steps).max()),
                 "reserve_probe": reserve_probe, "preflight": preflight,
                 "projected": scaling_projection_for(args.workload, args.graph, world),
                 "rccl_env": {k: os.environ.get(k) for k in ("NCCL_MAX_NCHANNELS", "NCCL_MIN_NCHANNELS", "NCCL_MAX_P2P_NCHANNELS")},
                 "note": "halo = one all-to-all-v of h (forward) and one of grad (backward) per epoch, " + str(DIMS[1]) + " floats per ghost row; "
                         "ms are HIP-event times on the comm stream (pack + grouped ncclSend/ncclRecv + unpack), overlapped with the interior-source SpMM blocks"}

    if gat or tf_mode or args.workload != "reddit":   # the roofline bookkeeping above is for the Reddit GCN epoch's three launches
        roofline = None
        roofline_gemm = None
    scale_name = {"reddit": "Reddit-scale"}.get(args.workload, args.workload + "-scale")
    if rank == 0:
        out = {
            "metric": (f"full-graph GAT ({'8-head extension' if args.gnn == 'gatmh' else 'reference prototype'}) epoch: "
                       f"aggregated edges/sec, {scale_name} synthetic" if gat else
                       f"full-graph GCN epoch: aggregated edges/sec (epoch time in ms_per_step), {scale_name} synthetic, "
                       f"{len(DIMS) - 1}-layer {'-'.join(map(str, DIMS))}"),
            "value": value, "unit": "edges/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
            "dtype": "f32", "data": "synthetic",
            "config": {"workload": ("Reddit GAT 2-layer 8-head, per-edge attention softmax (extension) full-graph" if args.gnn == "gatmh" else
                                    "Reddit GAT 2-layer (reference single-head prototype) full-graph" if gat else
                                    "Reddit GCN 2-layer (232965 verts, ~114.6M edges, feat 602-128-41) full-graph"
                                    if args.workload == "reddit" else
                                    f"{args.workload} GCN {len(DIMS) - 1}-layer ({V} verts, feat {'-'.join(map(str, DIMS))}) scale test"),
                       "graph": args.graph, "vertices": V, "edges": E_in, "options": args.opt or None,
                       "layer0_order": "transform-first A(XW) [opt-in, not the reference order]" if tf_mode else "aggregate-first (AX)W",
                       "partitioning": f"contiguous x{world}" + (f" (emulating rank {args.emulate}, no exchange)" if args.emulate else ""),
                       "transport": "RCCL over xGMI" if world > 1 and not host_tx else ("host callbacks over gloo (dry run of the N > 1 logic, not the metric)" if world > 1 else None),
                       "epoch_ms_min": float(np.min(epoch_ms)), "epoch_ms_median": float(np.median(epoch_ms))},
            "roofline": roofline,
            "roofline_gemm": roofline_gemm,
            "transform_first": alt,
            "cached_ah0": cached,
            "spmm_gates": gates,
            "cpu_baseline": cpu,
            "parity_unpinned": PARITY_UNPINNED,
            "kernel_ms_per_epoch": {k: round(v[0] / args.steps, 4) for k, v in fam.items() if v[1]},
            "halo_selfcheck": halo_ok, "halo_overlap": bool(world > 1), "multi_gpu": multi,
            "multi_gpu_on_record": multi_gpu_on_record() if world == 1 else None,
            "setup_s": round(t_setup, 1),
        }
    eng.close()
    ctx.close()
    # ---- the other single-GPU configurations, each timed the same way (extra keys beside the headline) ----
    if args.full and rank == 0 and world == 1 and not gat and not tf_mode and not args.emulate and not args.opt and not args.no_alt \
            and args.workload == "reddit" and args.graph == "uniform" and args.scale == 1.0:
        steps_x, warm_x = max(2, min(args.steps, 5)), 1
        out["gatmh"] = extra_epoch(da, part, g, "gatmh", V, steps_x, warm_x,
                                   "BASELINE config 3 wording: Reddit GAT 2-layer 8-head, per-edge attention softmax + weighted sum "
                                   "(extension, parity unpinned: the reference has no such kernel), same uniform graph")
        out["gat"] = extra_epoch(da, part, g, "gat", V, steps_x, warm_x,
                                 "BASELINE config 3, reference GAT prototype (single head, per-destination edge score), same uniform graph")
        del part
        src, dst = synth_edges("rmat", V, E_target)
        part_r = da.Partition.build(src, dst, np.zeros(V, np.int32), 0, 1)
        del src, dst
        out["rmat"] = extra_epoch(da, part_r, part_r.view(), "gcn", V, steps_x, warm_x,
                                  "same GCN epoch on an R-MAT graph (a=.57 b=.19 c=.19, SURVEY 8d): same V and E, max degree ~8e5")
        del part_r
        src, dst = synth_edges("community", V, E_target)
        part_c = da.Partition.build(src, dst, np.zeros(V, np.int32), 0, 1)
        del src, dst
        out["community"] = extra_epoch(da, part_c, part_c.view(), "gcn", V, steps_x, warm_x,
                                       "same GCN epoch on a graph with locality: 50 communities of consecutive ids, 85 % of the edges inside "
                                       "(a METIS-ordered Reddit seen from the kernels).  K1s's even layout spreads the communities away by "
                                       "construction; why a locality-keeping layout was not built: DESIGN.md section 3, round 4")
        del part_c
        out["amazon_rank0of8"] = rank_of_8_epoch(da, "amazon", max(5, steps_x), warm_x)
        if args.with_friendster:
            out["friendster_rank0of8"] = rank_of_8_epoch(da, "friendster", max(5, steps_x), warm_x)
    if rank == 0:
        print(json.dumps(out), flush=True)
    if world > 1:
        dist.destroy_process_group()


def rank_of_8_epoch(da, workload, steps, warmup):
    """BASELINE configs 4 / 5 as ONE rank of the 8-GPU run holds them (rank 0 of a contiguous 8-way split of the uniform
    synthetic graph of the real size; compute only -- no peers, so no exchange: the layer-0 ghost rows are resident like
    fg@0 from file, deeper ghost tensors are whatever they were).  Same epoch loop and timing as the headline."""
    Vw, Ew, dims = WORKLOADS[workload]
    t0 = time.time()
    src, dst = synth_incident_edges(Vw, Ew, 0, 8)
    parts = (np.arange(Vw, dtype=np.int64) * 8 // Vw).astype(np.int32)
    part = da.Partition.build(src, dst, parts, 0, 8)
    del src, dst, parts
    what = {"amazon": "BASELINE config 4 (Amazon GCN 3-layer 300-64-64-25, 9.43 M vertices, 231.6 M edges) as rank 0 of 8 holds it",
            "friendster": "BASELINE config 5 (Friendster GCN 2-layer 256-48-51, 65.6 M vertices, 3.61 G edges) as rank 0 of 8 holds it"}[workload]
    res = extra_epoch(da, part, part.view(), "gcn", Vw, steps, warmup,
                      what + ": uniform synthetic graph, only the records incident to the rank's block generated, compute only", dims=dims, ghosts=True,
                      pmc_key=workload + "_rank0of8")
    res["setup_s"] = round(time.time() - t0, 1)
    part.close()
    return res


def first_contact_preflight(da, dist, torch, rank, world, dev, host_tx, tdev):
    """N > 1, before any partition is built: the two collectives of the path on a 64-vertex-per-rank toy partition, through
    the same C-ABI calls the epoch uses -- a grouped ncclSend/ncclRecv exchange of 1 MB per peer (dory_halo_exchange, both
    directions) and a 311 KB ncclAllReduce (dory_weight_update) -- under a per-stage watchdog (DORY_PREFLIGHT_STAGE_S, 120 s) that
    names the call it was in and the seconds every earlier stage took.
    A first run on real xGMI then fails here, in seconds and with the failing call's name, not minutes later inside a
    timed region.  Results are checked (ghost rows bit-equal to the owners', gradient sum exact).  Over --transport host the
    same calls run with the bytes through gloo."""
    import threading
    stage = {"name": "start", "t0": time.time()}
    done = threading.Event()

    # the limit is PER STAGE (re-armed by enter()): a slow but healthy cold start -- RCCL's topology detection and lazy channel
    # setup on eight GPUs -- is many stages of a few seconds each, a hang is one stage that never ends
    limit = float(os.environ.get("DORY_PREFLIGHT_STAGE_S", "120"))
    stage["log"] = []

    def watchdog():
        while not done.wait(1.0):
            if time.time() - stage["t0"] > limit:
                sys.stderr.write("bench.py preflight: rank %d STUCK for %.0f s in: %s (stages before it: %s)\n"
                                 % (rank, time.time() - stage["t0"], stage["name"], "; ".join("%s %.1f s" % t for t in stage["log"])))
                sys.stderr.flush()
                os._exit(3)
    threading.Thread(target=watchdog, daemon=True).start()

    def enter(name):
        stage["log"].append((stage["name"], time.time() - stage["t0"]))
        stage["name"] = name
        stage["t0"] = time.time()
    n, dims = 64, [19, 4096, 4]                     # 64 rows x 4096 floats = 1 MB per peer; dW0 = 19 x 4096 floats = 311 KB
    V = n * world
    v = np.arange(V, dtype=np.uint32)
    nxt = ((v + n) % V).astype(np.uint32)           # vertex i of block r <-> vertex i of block r + 1: a ring of blocks
    src, dst = np.concatenate([v, nxt]), np.concatenate([nxt, v])
    parts = (v // n).astype(np.int32)
    t0 = time.time()
    enter("dory_partition_build (toy ring partition)")
    part = da.Partition.build(src, dst, parts, rank, world)
    g = part.view()
    ctx = da.Context(dev)
    ctx.configure(da.GCN, dims, V, rank, world)
    part.upload(ctx, parts)
    ctx.preallocate()
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    if host_tx:
        set_gloo_transport(ctx, dist, torch, rank, world)
    else:
        enter("ncclGetUniqueId + broadcast of the id (torch.distributed)")
        idt = torch.zeros(128, dtype=torch.uint8, device="cuda")
        if rank == 0:
            idt.copy_(torch.from_numpy(ctx.comm_unique_id()))
        with stdout_to_stderr():
            dist.broadcast(idt, 0)
            enter("dory_comm_init (ncclCommInitRank, %d ranks)" % world)
            ctx.comm_init(idt.cpu().numpy(), rank, world)
    res = {"vertices_per_rank": n, "bytes_per_peer": n * dims[1] * 4, "allreduce_bytes": dims[0] * dims[1] * 4}
    enter("dory_halo_exchange(layer 1, FORWARD): grouped ncclSend/ncclRecv, 1 MB per peer")
    ctx.fill_uniform(0, "h", 7, -1.0, 1.0, g["localToGlobal"])
    t1 = time.time()
    ctx.halo_exchange(1, da.FORWARD)
    ctx.sync()
    res["halo_forward_s"] = round(time.time() - t1, 4)
    ok = np.array_equal(ctx.download(1, "fg"), splitmix_uniform(7, g["srcGhost"], dims[1]))
    enter("dory_halo_exchange(layer 1, BACKWARD): grouped ncclSend/ncclRecv, 1 MB per peer")
    ctx.fill_uniform(1, "grad", 9, -1.0, 1.0, g["localToGlobal"])
    t1 = time.time()
    ctx.halo_exchange(1, da.BACKWARD)
    ctx.sync()
    res["halo_backward_s"] = round(time.time() - t1, 4)
    ok = ok and np.array_equal(ctx.download(0, "bg"), splitmix_uniform(9, g["dstGhost"], dims[1]))
    enter("dory_weight_update(layer 0): ncclAllReduce(sum) of 311 KB + Adam")
    ctx.weight_grad_set(0, np.full((dims[0], dims[1]), float(rank + 1), np.float32))
    t1 = time.time()
    ctx.weight_update(0)
    ctx.sync()
    res["allreduce_adam_s"] = round(time.time() - t1, 4)
    ok = ok and bool(np.all(ctx.weight_grad_get(0) == np.float32(world * (world + 1) / 2)))
    enter("closing the toy context (ncclCommDestroy)")
    ctx.close()
    part.close()
    enter("torch.distributed all_reduce of the verdict")
    flag = torch.tensor([1 if ok else 0], dtype=torch.int32, device=tdev)
    dist.all_reduce(flag, op=dist.ReduceOp.MIN)
    done.set()
    res["ok"] = bool(flag.item())
    res["seconds"] = round(time.time() - t0, 2)
    res["stage_seconds"] = {n_: round(t_, 3) for n_, t_ in stage["log"][1:]}
    res["transport"] = "host callbacks over gloo" if host_tx else "RCCL"
    if not res["ok"]:
        raise SystemExit("bench.py preflight FAILED on rank %d: exchanged ghost rows or the gradient sum are wrong (%r)" % (rank, res))
    return res


def extra_epoch(da, part, g, gnn, V, steps, warmup, what, dims=None, ghosts=False, pmc_key=None):
    """one more configuration on one GPU: fresh context, same epoch loop, K timed steps after W warm-up steps"""
    import torch
    DIMS_ = dims or DIMS
    N = int(g["localVtxCnt"])
    ctx = da.Context(0)
    gat = gnn in ("gat", "gatmh")
    ctx.configure({"gcn": da.GCN, "gat": da.GAT, "gatmh": da.GATMH}[gnn], DIMS_, V, 0, 1)
    if gnn == "gatmh":
        ctx.gatmh_heads([8, 1])
    part.upload(ctx, None)
    ctx.preallocate()
    ctx.fill_uniform(0, "h" if gat else "x", 1, -1.0, 1.0, g["localToGlobal"])
    if ghosts and int(g["srcGhostCnt"]) and not gat:          # one rank of a P-way split alone: layer-0 ghost rows "from file"
        ctx.fill_uniform(0, "fg", 1, -1.0, 1.0, g["srcGhost"])
    labels = np.random.default_rng(2).integers(0, DIMS_[-1], V).astype(np.uint32)
    ctx.labels_upload(labels[g["localToGlobal"]])
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    eng = da.NativeEngine(ctx)
    eng.run(warmup)
    ctx.timing_reset()
    ctx.timing_enable(True)
    ctx.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(steps)
    ctx.sync()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / steps
    fam = {f: ctx.timing_get(f) for f in ("spmm", "gemm", "loss", "adam")}
    nnz_in, nnz_out = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])
    nl_ = len(DIMS_) - 1
    edges = (4 * nnz_in + 2 * nnz_out) if gat else (nl_ * nnz_in + (nl_ - 1) * nnz_out)
    res = {"what": what, "ms_per_step": ms, "steps": steps, "warmup": warmup, "edges_per_s": edges / (ms * 1e-3),
           "spmm_variant": ctx.get_option("spmm_variant"),
           "kernel_ms_per_epoch": {k: round(v[0] / steps, 4) for k, v in fam.items() if v[1]}}
    if gnn == "gat":
        # edges_per_s counts the reference's SIX aggregations per epoch (2 forward + 2 x 2 backward); with gat_reuse_nsum the
        # backward's dA-weighted one is a row-wise kernel on the forward's neighbour sum: four edge sweeps run
        reuse = bool(ctx.get_option("gat_reuse_nsum"))
        res["aggregations_counted_per_epoch"] = 6
        res["edge_sweeps_per_epoch"] = 4 if reuse else 6
        res["gat_reuse_nsum"] = reuse
    if gnn == "gcn" and dims is not None and fam["spmm"][1]:
        # roofline of this partition's aggregations (K1 row gather on partitions of this size: HBM / fabric bound):
        # compulsory bytes of the epoch's 2L-1 launches over their HIP-event time, and the gathered row bytes
        # against the ~6.3 TB/s a streaming kernel achieves on this HBM (MI355X_MICROARCH.md)
        Gs_, Gd_ = int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
        algo = sum(spmm_algorithmic_bytes(N, Gs_, nnz_in, DIMS_[l]) for l in range(nl_)) + \
            sum(spmm_algorithmic_bytes(N, Gd_, nnz_out, DIMS_[l]) for l in range(1, nl_))
        gathered = 4 * (sum(nnz_in * ((DIMS_[l] + 31) // 32 * 32) for l in range(nl_)) +
                        sum(nnz_out * ((DIMS_[l] + 31) // 32 * 32) for l in range(1, nl_)))
        t = fam["spmm"][0] / steps * 1e-3
        res["partition"] = {"local_vertices": N, "src_ghosts": Gs_, "dst_ghosts": Gd_, "in_edges": nnz_in, "out_edges": nnz_out}
        traffic_, traffic_src_ = None, "no PMC pass on record for this configuration"
        try:     # HBM-side bytes per epoch from the separate --pmc FETCH_SIZE pass (profiles/), for the kernel source it was collected for
            ent = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get(pmc_key or "", None)
            if ent and ent.get("spmm_hip_blob") == spmm_source_stamp():
                traffic_, traffic_src_ = ent.get("bytes_per_epoch", ent["fetch_bytes_per_epoch"]), ent["source"]
            elif ent:
                traffic_src_ = "stale: collected for another spmm.hip -- re-run tools/collect_profiles.sh"
        except (OSError, KeyError, ValueError):
            pass
        res["roofline"] = {"bound": "hbm", "achieved": round(algo / t / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                           "frac": round(algo / t / 1e9 / 8000.0, 5), "traffic": traffic_, "traffic_source": traffic_src_,
                           "traffic_what": "HBM-side bytes per epoch (2 x FETCH_SIZE + WRITE_SIZE of all its aggregation launches; FETCH only where no WRITE pass is on record); algorithmic_bytes_per_epoch is the figure `achieved` uses",
                           "kernel": "spmm_rows_kernel<GROUP,CHUNKS> (K1 row gather; %d launches per epoch)" % (2 * nl_ - 1),
                           "algorithmic_bytes_per_epoch": int(algo), "aggregation_ms_per_epoch": round(t * 1e3, 4),
                           "gathered_bytes_per_epoch": int(gathered), "gathered_TBps": round(gathered / t / 1e12, 3),
                           "gathered_frac_of_achievable_hbm_6.3_TBps": round(gathered / t / 1e12 / 6.3, 4)}
    if gnn == "gatmh" and fam["spmm"][1]:
        # compulsory bytes of the epoch's FOUR edge passes (round 5: forward over the CSC and source-side backward over the CSR
        # of both layers; the destination-side backward pass is a row-wise kernel since the forward carries the positive-branch
        # sums), each: the index stream once + pointers + one read and one write of an N x ld row tensor (z / dO in, o / dz
        # out) + the per-(vertex, head) scores and statistics (K floats x 4 per row); plus the row-wise stage's three reads
        # of an N x ld tensor (dO, o, op) and the forward's second output (op)
        lds = [(DIMS_[1] + 31) // 32 * 32, (DIMS_[2] + 31) // 32 * 32]
        swept = bool(ctx.get_option("gatmh_sweep"))
        algo = 0
        for ld_, K_ in ((lds[0], 8), (lds[1], 1)):
            for nnz in (nnz_in, nnz_out):
                algo += 4 * nnz + 8 * (N + 1) + 2 * 4 * N * ld_ + 4 * 4 * N * K_
            algo += 4 * 4 * N * ld_
        gathered = 4 * (nnz_in + nnz_out) * (lds[0] + lds[1])
        t = fam["spmm"][0] / steps * 1e-3
        traffic_, traffic_src_ = None, "no PMC pass on record for this build of the sweep kernels"
        try:     # HBM-side bytes of the epoch's sweep kernels: separate --pmc FETCH_SIZE / WRITE_SIZE passes (tools/collect_profiles.sh)
            ent = json.load(open(os.path.join(ROOT, "profiles", "pmc_traffic.json"))).get("gatmh_sweeps", None)
            if ent and swept and ent.get("source_stamp") == source_stamp(GATMH_STAMP_FILES):
                traffic_, traffic_src_ = ent["bytes_per_epoch"], ent["source"]
            elif ent:
                traffic_src_ = "stale: collected for another gat_mh_sweep.hip / sweep_core.hpp -- re-run tools/collect_profiles.sh"
        except (OSError, KeyError, ValueError):
            pass
        res["roofline"] = {"bound": "hbm", "achieved": round(algo / t / 1e9, 2), "peak": 8000.0, "unit": "GB/s",
                           "frac": round(algo / t / 1e9 / 8000.0, 5), "traffic": traffic_, "traffic_source": traffic_src_,
                           "traffic_what": "HBM-side bytes per epoch of the four sweep kernels (2 x FETCH_SIZE + WRITE_SIZE, separate --pmc passes)",
                           "algorithmic_bytes_per_epoch": int(algo), "aggregation_ms_per_epoch": round(t * 1e3, 4),
                           "kernel": ("gatmh_forward_sweep_kernel + gatmh_src_sweep_kernel on K1s's skeleton (four edge passes per epoch: single-pass "
                                      "softmax against an upper-bound shift; t / der row-wise from the forward's positive-branch sums)") if swept else
                                     "gatmh_*_blocked_kernel family + reduce kernels (six edge passes per epoch)",
                           "edge_passes_per_epoch": 4 if swept else 6,
                           "gathered_bytes_per_epoch": int(gathered if swept else 4 * (3 * nnz_in * lds[0] + 3 * nnz_in * lds[1])),
                           "l1_path_frac": round((gathered if swept else 4 * (3 * nnz_in * lds[0] + 3 * nnz_in * lds[1])) / t / 1e12 / 37.7, 4),
                           "note": "round 4's line counted six passes (3.94 GB, 264 GB gathered); with the sweep forms the epoch needs four: "
                                   "achieved / frac are against the four-pass figure, l1_path_frac against the rows actually gathered"}
    if gnn == "gcn" and dims is not None:
        # the same partition in the transform-first order (opt-in gcn_transform_first=2, not the reference's schedule): the layers
        # whose input is wider than their output gather the narrower rows -- on config 4 the 300-float launch becomes a 64-float one
        ctx.set_option("gcn_transform_first", 2)
        if ctx.transform_first_active():
            ctx.timing_enable(False)
            eng.run(1)
            ctx.sync()
            t1 = time.perf_counter()
            eng.run(steps)
            ctx.sync()
            res["transform_first"] = {"ms_per_step": (time.perf_counter() - t1) * 1e3 / steps,
                                      "what": "opt-in gcn_transform_first=2 on the same partition (z_l = A(in_l W_l) where the layer narrows); "
                                              "not the reference order, not the figure above"}
        ctx.set_option("gcn_transform_first", 0)
    eng.close()
    ctx.close()
    return res


def scaling_projection_for(workload, graph, world):
    """The epoch this repo expected of a `world`-GPU run BEFORE it ran (tools/scaling_projection.py, written in round 5 from
    per-rank measurements on one GPU + 153 GB/s per xGMI link): printed beside the measurement so that the first real
    multi-GPU record carries prediction and measurement side by side."""
    try:
        src = next(f for f in ("r06_scaling_projection.json", "r05_scaling_projection.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
        pj = json.load(open(os.path.join(ROOT, "profiles", src)))
        case = pj["cases"][f"{workload}:{graph}"]
        e = case["by_P"][str(world)]
        return {"available": True, "source": f"profiles/{src} (tools/scaling_projection.py; projection, not a measurement)",
                "projected_epoch_ms": e["projected_epoch_ms"], "compute_ms_max_rank": e["compute_ms_max"], "compute_ms_mean": e["compute_ms_mean"],
                "exposed_halo_ms_max_rank": e["exposed_halo_ms_max"], "allreduce_ms": e["allreduce_ms"],
                "halo_bytes_per_exchange_max_peer": e["halo_bytes_per_exchange_max_peer"], "nnz_in_max_over_mean": e["nnz_in_max_over_mean"],
                "single_gpu_epoch_ms": case.get("single_gpu_epoch_ms"), "projected_speedup": e.get("projected_speedup"),
                "model": e["model"]}
    except (OSError, KeyError, ValueError, StopIteration) as ex:
        return {"available": False, "why": f"no projection on record for {workload}:{graph} x{world} ({type(ex).__name__})"}


def multi_gpu_on_record():
    """What this repo has on record about N > 1 when the line itself is a 1-GPU run (no multi-GPU node has been available):
    the projected epochs (tools/scaling_projection.py) and the overlapped halo schedule measured with real concurrency on ONE
    GPU (P ranks of one process over dory_comm_init_local, tools/local_transport_run.py).  Pointers into profiles/, not
    measurements of this run."""
    rec = {"note": "from profiles/ (committed evidence), not measured by this run; no RCCL call has run with more than one rank"}
    try:
        src = next(f for f in ("r06_scaling_projection.json", "r05_scaling_projection.json") if os.path.exists(os.path.join(ROOT, "profiles", f)))
        pj = json.load(open(os.path.join(ROOT, "profiles", src)))["cases"]
        rec["projected_epoch_ms"] = {c: {P: v["projected_epoch_ms"] for P, v in r["by_P"].items()} for c, r in pj.items()}
        rec["projection_source"] = "profiles/" + src
    except (OSError, KeyError, ValueError, StopIteration):
        pass
    try:
        lt = json.load(open(os.path.join(ROOT, "profiles", "r06_local_transport.json")))
        rec["overlap_on_one_gpu"] = [{k: r[k] for k in ("config", "P", "halo_overlap", "epoch_ms_median_max_rank", "halo_overlap_fraction",
                                                         "identical_bits_overlap_on_off")} |
                                     {"gate_timeouts": sum(g["timeouts"] for g in r["spmm_gates"])} for r in lt["runs"]]
        rec["overlap_source"] = "profiles/r06_local_transport.json"
    except (OSError, KeyError, ValueError):
        pass
    return rec


def set_gloo_transport(ctx, dist, torch, rank, world):
    """--transport host: the bytes of the halo exchange and of the gradient sum through gloo (tests/test_gpu_multirank.py
    does the same around dory_engine_run); everything else of the multi-rank path stays the library's."""
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


class stdout_to_stderr:
    """RCCL prints a line ("Librccl path : ...") on stdout when a communicator is created; the driver reads the JSON
    line from stdout, so file descriptor 1 points at stderr while communicators are being set up."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)
        return False


def usable_cpus():
    """hardware threads this process may really use: affinity mask capped by the cgroup
    CPU quota (the GPU box shows 256 CPUs but grants 16 via cpu.max)."""
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except (OSError, ValueError):
        pass
    return n


def cpu_baseline(ctx, g, rows):
    """Times oracle/ (the CPU restatement of the reference's cpu backend: aggregateGCN +
    CPUComm::vtxNN*GCN) on this box's host cores over ONE FULL EPOCH of the same graph and
    the same inputs the GPU run used: all rows, three aggregations through the per-edge
    pointer tables of engine/utils.cpp:655-705 (built before the clock starts, as the
    reference builds them in preallocate), five GEMMs, activations and loss.  OpenMP over
    vertices with the default (static) schedule like gcn_ops.cpp:159-161, one fixed thread
    count = the hardware threads this process may use.  `rows` > 0 restricts the epoch to
    the first `rows` destination rows (diagnostic).  Reported, not optimised against."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import orc
    N = int(g["localVtxCnt"])
    V = int(g["globalVtxCnt"])
    ncores = usable_cpus()
    full = rows <= 0 or rows >= N
    rows = N if full else rows
    orc.lib.orc_set_threads(ncores)

    def sub(ptr_key, idx_key, val_key):
        ptr = np.ascontiguousarray(g[ptr_key][:rows + 1])
        e = int(ptr[-1])
        return ptr, np.ascontiguousarray(g[idx_key][:e]), np.ascontiguousarray(g[val_key][:e]), e
    cptr, cidx, cval, e_in = sub("colPtr", "rowIdx", "cscVal")
    rptr, ridx, rval, e_out = sub("rowPtr", "colIdx", "csrVal")
    norm = np.ascontiguousarray(g["norm"][:rows])
    X = np.ascontiguousarray(ctx.download(0, "x"))            # the very inputs / intermediates of the GPU run
    H = np.ascontiguousarray(ctx.download(0, "h"))
    G1 = np.ascontiguousarray(ctx.download(1, "grad"))
    lab = ctx.download(1, "lab")[:rows]
    # weights as they were when the last GPU epoch started are gone (Adam stepped);
    # the baseline only needs *a* weight set of the right shape for timing + ah parity
    W0, W1 = ctx.weight_get(0), ctx.weight_get(1)

    def agg(ptr, idx, val, Xfull):
        # pointer table first (not timed: preallocate-time work in the reference), then the timed aggregation
        F = Xfull.shape[1]
        tail = Xfull[rows:] if rows < N else None                 # "ghost" rows = rest of the buffer (sampled runs)
        eptr, keep = orc.edge_pointers(ptr, idx, Xfull[:rows], tail)
        t0 = time.perf_counter()
        out = orc.aggregate_gcn_ptr(ptr, eptr, val, norm, Xfull[:rows])
        dt = time.perf_counter() - t0
        del eptr, keep
        return out, dt
    stage = {}
    ah0, stage["agg_F602"] = agg(cptr, cidx, cval, X)                            # GA  L0 fwd
    t0 = time.perf_counter()
    z0, h0 = orc.vtx_forward_hidden(ah0, W0)                                      # AV  L0 fwd
    stage["transform_L0"] = time.perf_counter() - t0
    ah1, stage["agg_F128_fwd"] = agg(cptr, cidx, cval, H)                        # GA  L1 fwd
    t0 = time.perf_counter()
    orc.vtx_forward_last(ah1, W1, lab, V)                                         # AV  L1 fwd (+loss, grad, dW1)
    stage["transform_last"] = time.perf_counter() - t0
    aTg0, stage["agg_F128_bwd"] = agg(rptr, ridx, rval, G1)                      # GA  L1 bwd
    t0 = time.perf_counter()
    orc.vtx_backward(aTg0, z0, ah0, W0, 0)                                        # AV  L0 bwd (dW0)
    stage["transform_bwd"] = time.perf_counter() - t0
    total = sum(stage.values())
    edges = 2 * e_in + e_out
    gpu_ah0 = ctx.download(0, "ah")[:rows]
    err = float(np.abs(gpu_ah0 - ah0).max() / max(np.abs(ah0).max(), 1e-30))
    what = "one FULL epoch of the same graph (all %d rows" % rows if full else "one epoch restricted to the first %d destination rows (" % rows
    return {"value": edges / total, "unit": "edges/s", "cores": ncores, "kind": "port",
            "sample": f"{what}, {e_in} in-edges, {e_out} out-edges): 3 aggregations through per-edge pointer tables "
                      f"(engine/utils.cpp:655-705, built outside the clock) + 5 GEMMs + activations/loss, "
                      f"{total:.2f} s of CPU time = epoch_s, OpenMP static over vertices, {ncores} threads (all this process may use)",
            "epoch_s": round(total, 3),
            "stage_s": {n: round(v, 3) for n, v in stage.items()},
            "gpu_vs_oracle_rel_err_ah0": err}


if __name__ == "__main__":
    main()
