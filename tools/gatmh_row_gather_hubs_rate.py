#!/usr/bin/env python3
"""What does hub splitting buy the multi-head GAT's row-gather kernels (csrc/gat_mh_rows.hip, dory_gatmh_row_gather_hub_split)?

Inputs: rank 0 of 8 (contiguous blocks) of an R-MAT graph at Amazon size from bench.py's own generator (synth_edges("rmat")) -- the
power-law case the feature is for -- and rank 0 of 8 of the uniform graph of that size (synth_incident_edges) as the control.  Compute
only, as tools/gatmh_row_gather_rate.py runs it: the ghost tensors are filled once and never exchanged, dory_gatmh_row_gather(1).
Two models: 300-128-41 with heads 8 / 1 (128- and 64-float rows; both destination sides are the row-wise kernel: no edges) and 300-64-25
with heads 32 / 1 (64- and 32-float rows; both destination sides are the edge pass).

Per layer and pass the device time of single dory_aggregate calls (the library's timing family around the pass) for
  parent   the library given with --parent-lib (a build of the parent commit),
  off      this library, chunk_entries = 0,
  1024 / 2048 / 4096 / 8192   this library, that chunk size,
the two libraries alternated over --rounds rounds (one child process per input, model, library and round; this library's child runs
its settings in turn on one context).  Then per line the median and the spread (min .. max) over the rounds, the ratio to the parent's
median, and whether the medians differ by more than the larger of the two spreads.
Every child runs under a time limit; the first that fails or runs out of time ends the run.
GPU box only:  python tools/gatmh_row_gather_hubs_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 300]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
MODELS = {"8x16": ([300, 128, 41], [8, 1]), "32x2": ([300, 64, 25], [32, 1])}
CHUNKS = (1024, 2048, 4096, 8192)


def timed(ctx, fam, fn, calls):
    fn()
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(calls):
        fn()
    ctx.sync()
    ms, n = ctx.timing_get(fam)
    ctx.timing_enable(False)
    assert n, fam
    return ms / calls


def rate_child(graph, model, lib, path, calls):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import WORKLOADS
    from gatmh_row_gather_rate import gatmh_ctx
    V = WORKLOADS["amazon"][0]
    part = da.Partition.load(path)
    dims, heads = MODELS[model]
    ctx, g = gatmh_ctx(da, part, dims, heads, V, 1, {})
    eng = da.NativeEngine(ctx)      # one epoch: every tensor the single passes below read is current
    eng.run(1)
    ctx.sync()
    eng.close()
    for arm in (("parent",) if lib == "parent" else ("off",) + CHUNKS):
        if lib != "parent":
            ctx.gatmh_row_gather_hub_split(0 if arm == "off" else arm)
            st = ctx.gatmh_row_gather_hub_split_stats()
            print("PLAN %s %s %s in_hub_rows %d in_chunks %d out_hub_rows %d out_chunks %d" %
                  (graph, model, arm, st["in_hub_rows"], st["in_chunks"], st["out_hub_rows"], st["out_chunks"]))
        for layer in (1, 2):
            K = heads[layer - 1]
            zw = dims[layer] * (K if layer == 2 else 1)
            tag = "%s %s %s layer%d %dx%d" % (graph, model, arm, layer, K, zw // K)
            before = ctx.gatmh_row_gather_stats()
            print("RATE %s forward ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.FORWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 1)
            ctx.aggregate(layer, da.BACKWARD)
            d = [a - b for a, b in zip(ctx.gatmh_row_gather_stats(), before)]
            if d[1] > 0:
                print("RATE %s dst_edge_pass ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 2)
            print("RATE %s src ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 0)
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="a build of the parent commit (arm `parent`); without it that arm runs this tree's library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        rate_child(a.child[0], a.child[1], a.child[2], a.child[3], int(a.child[4]))
        return
    import dorylus_amd as da
    from bench import WORKLOADS, synth_edges, synth_incident_edges
    lines = []

    def say(ln):
        print(ln, flush=True)
        lines.append(ln)

    def step(args, lib):
        env = dict(os.environ)
        if lib:
            env["DORY_LIB_PATH"] = os.path.abspath(lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True,
                               timeout=a.step_timeout, env=env)
        except subprocess.TimeoutExpired:
            print("# step %s ran out of time: stopping" % (args,), flush=True)
            return False
        for ln in r.stdout.splitlines():
            if ln.split(" ")[0] in ("RATE", "PLAN"):
                say(ln)
        if r.returncode != 0:
            print("# step %s failed (%d): stopping\n%s" % (args, r.returncode, r.stderr[-2000:]), flush=True)
        return r.returncode == 0

    with tempfile.TemporaryDirectory() as tmp:
        V, E, _ = WORKLOADS["amazon"]
        parts = (np.arange(V, dtype=np.int64) * 8 // V).astype(np.int32)
        paths = {}
        for graph in ("rmat", "uniform"):
            t0 = time.time()
            if graph == "rmat":
                src, dst = synth_edges("rmat", V, E)
                keep = (parts[src] == 0) | (parts[dst] == 0)          # the records rank 0 needs (the builder skips the others anyway)
                src, dst = src[keep], dst[keep]
            else:
                src, dst = synth_incident_edges(V, E, 0, 8)
            print("# %s: records of rank 0 generated, %.0f s" % (graph, time.time() - t0), flush=True)
            part = da.Partition.build(src, dst, parts, 0, 8)
            del src, dst
            g = part.view()
            din, dout = np.diff(np.asarray(g["colPtr"], np.int64)), np.diff(np.asarray(g["rowPtr"], np.int64))
            say("PART %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d max_in_degree %d max_out_degree %d rows_over_1024 %d / %d" %
                (graph, int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"]), int(g["localInEdgeCnt"]),
                 int(g["localOutEdgeCnt"]), int(din.max()), int(dout.max()), int((din > 1024).sum()), int((dout > 1024).sum())))
            paths[graph] = os.path.join(tmp, graph + ".part")
            part.save(paths[graph])
            part.close()
            print("# %s: partition built and saved, %.0f s" % (graph, time.time() - t0), flush=True)
        ok = True
        for rnd in range(a.rounds):
            for graph in ("rmat", "uniform"):
                for model in MODELS:
                    for lib, so in (("parent", a.parent_lib), ("this", "")):
                        ok = ok and step([graph, model, lib, paths[graph], str(a.calls)], so)
            if not ok:
                break
    # per line: median and spread over the rounds; against the parent
    med = {}
    for ln in lines:
        if ln.startswith("RATE "):
            w = ln.split()
            med.setdefault((w[1], w[2], w[4], w[5], w[6]), {}).setdefault(w[3], []).append(float(w[8]))     # graph, model, layer, shape, pass
    for key, arms in sorted(med.items()):
        if "parent" not in arms:
            continue
        p = arms["parent"]
        pm, ps = float(np.median(p)), max(p) - min(p)
        for arm in ("off",) + tuple(str(c) for c in CHUNKS):
            if arm not in arms:
                continue
            x = arms[arm]
            xm, xs = float(np.median(x)), max(x) - min(x)
            verdict = "inside the spread" if abs(xm - pm) <= max(ps, xs) else "FASTER" if xm < pm else "NOT FASTER"
            say("RATIO %s %s %s %s %s arm %s parent_ms %.4f (%.4f..%.4f) ms %.4f (%.4f..%.4f) over_parent %.3f  %s" %
                (key + (arm, pm, min(p), max(p), xm, min(x), max(x), xm / pm, verdict)))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
