#!/usr/bin/env python3
"""What do the multi-head GAT's row-gather kernels (csrc/gat_mh_rows.hip, dory_gatmh_row_gather) reach, against K1 on the same rows?

  1. Rank 0 of 8 of the Amazon-size uniform graph (built as bench.py's rank_of_8_epoch builds it; compute only: no peers, the ghost
     tensors are filled once and never exchanged), model 300-64-25 with heads 8 / 1 and with heads 32 / 1 -- both gather 64-float
     rows on the hidden layer; 8 x 8 takes the row-wise destination side, 32 x 2 the destination-side edge pass.  Mode 1 (the
     partition is alone on the device, so the context has one node).  The epoch, and per pass of the hidden layer the device time
     (the library's timing families around single dory_aggregate calls) and TB/s of gathered rows = edges x 4 ld bytes (the self
     edge, the edge ids and the per-edge score / statistics records are NOT counted: the rows are what K1 gathers too).
  2. The yardstick, same process series: K1 (spmm_variant = 0) aggregating 64-float rows over the same partition's in-edges.
  3. The Reddit-size graph, single partition, model 602-128-41 heads 8 / 1: mode 0 (the sweep forms), mode 1, and mode 0 with
     gatmh_sweep = 0, gatmh_blocked = 0 (the row-wise forms of round 1).
Every measurement is a child process of its own under a time limit; the first that fails or runs out of time ends the run.  The
partitions are built once by the parent (host only) and handed to the children as files.  Needs no file outside the tree.
GPU box only:  python tools/gatmh_row_gather_rate.py [--out FILE] [--step-timeout 300] [--skip-reddit]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
CALLS, STEPS, WARM = 10, 5, 2
AMAZON_DIMS, REDDIT_DIMS = [300, 64, 25], [602, 128, 41]
STEPS_LIST = (("amazon", "k1"), ("amazon", "rows:8"), ("amazon", "rows:32"), ("amazon", "k1"),
              ("reddit", "epoch:sweep"), ("reddit", "epoch:rows"), ("reddit", "epoch:rowwise"))


def timed(ctx, fam, fn):
    fn()
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(CALLS):
        fn()
    ctx.sync()
    ms, n = ctx.timing_get(fam)
    ctx.timing_enable(False)
    assert n, fam
    return ms / CALLS


def epoch_ms(ctx, da):
    import torch
    eng = da.NativeEngine(ctx)
    eng.run(WARM)
    ctx.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(STEPS)
    ctx.sync()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / STEPS
    eng.close()
    return ms


def gatmh_ctx(da, part, dims, heads, V, mode, opts):
    g = part.view()
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, V, 0, 1)
    ctx.gatmh_heads(heads)
    for k, v in opts.items():
        ctx.set_option(k, v)
    ctx.gatmh_row_gather(mode)
    part.upload(ctx, None)
    ctx.preallocate()
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
    for l in range(len(dims) - 1):          # the ghost rows nobody sends here: finite values, once
        if int(g["srcGhostCnt"]):
            ctx.fill_uniform(l, "fg_z", 2 + l, -1.0, 1.0)
            ctx.fill_uniform(l, "fg_el", 4 + l, -0.5, 0.5)
        if int(g["dstGhostCnt"]):
            ctx.fill_uniform(l, "bg_do", 6 + l, -1.0, 1.0)
            ctx.fill_uniform(l, "bg_st", 8 + l, 0.25, 1.0)
    labels = np.random.default_rng(2).integers(0, dims[-1], V).astype(np.uint32)
    ctx.labels_upload(labels[g["localToGlobal"]])
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    return ctx, g


def child(workload, what, path):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import WORKLOADS
    V = WORKLOADS[workload][0]
    part = da.Partition.load(path)
    g = part.view()
    nin, nout = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])
    print("PART %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d" %
          (workload, int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"]), nin, nout))
    if what == "k1":
        ctx = da.Context(0)
        ctx.configure(da.GCN, [64, 32, 25], V, 0, 1)
        ctx.set_option("spmm_variant", 0)
        part.upload(ctx, None)
        ctx.preallocate()
        ctx.fill_uniform(0, "x", 1, -1.0, 1.0, g["localToGlobal"])
        if int(g["srcGhostCnt"]):
            ctx.fill_uniform(0, "fg", 1, -1.0, 1.0, g["srcGhost"])
        ms = timed(ctx, "spmm", lambda: ctx.aggregate(0, da.FORWARD))
        assert ctx.get_option("spmm_launches_k1") > 0 and ctx.get_option("spmm_launches_k1s") == 0
        print("RATE k1 forward ld 64 ms %.4f gathered_TBps %.3f" % (ms, nin * 256 / ms / 1e9))
        ctx.close()
        return
    kind, arg = what.split(":")
    if kind == "rows":
        K = int(arg)
        ctx, g = gatmh_ctx(da, part, AMAZON_DIMS, [K, 1], V, 1, {})
        print("EPOCH amazon_rank0of8 heads %dx%d mode 1 ms %.3f" % (K, 64 // K, epoch_ms(ctx, da)))
        before = ctx.gatmh_row_gather_stats()
        fwd = timed(ctx, "spmm", lambda: ctx.aggregate(1, da.FORWARD))
        ctx.set_option("gatmh_bwd_phase", 1)
        ctx.aggregate(1, da.BACKWARD)
        d = [a - b for a, b in zip(ctx.gatmh_row_gather_stats(), before)]
        edge = d[1] > 0
        dst = timed(ctx, "spmm" if edge else "loss", lambda: ctx.aggregate(1, da.BACKWARD))
        ctx.set_option("gatmh_bwd_phase", 2)
        src = timed(ctx, "spmm", lambda: ctx.aggregate(1, da.BACKWARD))
        ctx.set_option("gatmh_bwd_phase", 0)
        print("RATE rows%d forward ld 64 ms %.4f gathered_TBps %.3f" % (K, fwd, nin * 256 / fwd / 1e9))
        if edge:
            print("RATE rows%d dst_edge_pass ld 64 ms %.4f gathered_TBps %.3f" % (K, dst, nin * 256 / dst / 1e9))
        else:
            print("RATE rows%d dst_rowwise ld 64 ms %.4f (family loss: the ELU backward and the row-wise kernel; no rows gathered)" % (K, dst))
        print("RATE rows%d src ld 64 ms %.4f gathered_TBps %.3f" % (K, src, nout * 256 / src / 1e9))
        ctx.close()
        return
    opts, mode = {"sweep": ({}, 0), "rows": ({}, 1), "rowwise": ({"gatmh_sweep": 0, "gatmh_blocked": 0}, 0)}[arg]
    ctx, g = gatmh_ctx(da, part, REDDIT_DIMS, [8, 1], V, mode, opts)
    ms = epoch_ms(ctx, da)
    print("EPOCH reddit single partition heads 8x16 %s ms %.3f row_gather_passes %s" % (arg, ms, ctx.gatmh_row_gather_stats()))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--skip-reddit", action="store_true")
    ap.add_argument("--child", nargs=3, metavar=("WORKLOAD", "WHAT", "PARTITION"))
    a = ap.parse_args()
    if a.child:
        child(*a.child)
        return
    import dorylus_amd as da
    from bench import WORKLOADS, synth_edges, synth_incident_edges
    lines = []
    with tempfile.TemporaryDirectory() as tmp:
        paths = {}
        for wl in ("amazon",) + (() if a.skip_reddit else ("reddit",)):
            V, E, _ = WORKLOADS[wl]
            t0 = time.time()
            if wl == "amazon":
                src, dst = synth_incident_edges(V, E, 0, 8)
                parts = (np.arange(V, dtype=np.int64) * 8 // V).astype(np.int32)
                part = da.Partition.build(src, dst, parts, 0, 8)
            else:
                src, dst = synth_edges("uniform", V, E)
                part = da.Partition.build(src, dst, np.zeros(V, np.int32), 0, 1)
            del src, dst
            paths[wl] = os.path.join(tmp, wl + ".part")
            part.save(paths[wl])
            part.close()
            print("# partition %s built in %.1f s" % (wl, time.time() - t0), flush=True)
        for wl, what in STEPS_LIST:
            if wl not in paths:
                continue
            cmd = [sys.executable, os.path.abspath(__file__), "--child", wl, what, paths[wl]]
            try:
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                print("# step %s %s ran out of time: stopping" % (wl, what), flush=True)
                break
            got = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("PART", "RATE", "EPOCH")]
            for ln in got:
                print(ln, flush=True)
            lines += got
            if r.returncode != 0:
                print("# step %s %s failed (%d): stopping\n%s" % (wl, what, r.returncode, r.stderr[-2000:]), flush=True)
                break
    k1 = [float(ln.split()[-1]) for ln in lines if ln.startswith("RATE k1 ")]
    if k1:
        ref = sorted(k1)[len(k1) // 2]
        for ln in lines:
            if ln.startswith("RATE rows") and "gathered_TBps" in ln:
                f = float(ln.split()[-1]) / ref
                out = "FRACTION_OF_K1 %s %s %.3f%s" % (ln.split()[1], ln.split()[2], f, "  (below half of K1)" if f < 0.5 else "")
                print(out, flush=True)
                lines.append(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
