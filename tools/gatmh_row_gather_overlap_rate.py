#!/usr/bin/env python3
"""What does running the interior rows beside the exchange cost and hide (csrc/gat_mh_rows.hip, dory_gatmh_row_gather_overlap)?

1. Compute only, one rank, nothing in flight (as tools/gatmh_row_gather_hubs_rate.py runs it: rank 0 of 8, contiguous blocks, of an
   Amazon-size graph; the ghost tensors are filled once and never exchanged; dory_gatmh_row_gather(1); model 300-128-41, heads 8 / 1):
     community   bench.py's synth_edges("community"): 50 communities of consecutive ids, 85 % of the edges inside,
     uniform     bench.py's synth_incident_edges -- the rank r25 - r28 measured.
   Per layer, the forward and the source side as single dory_aggregate calls (the library's timing family around the pass) for
     parent   the library given with --parent-lib (a build of the parent commit),
     off      this library, the switch off,
     on       this library, the switch on: two launches instead of one,
   the two libraries alternated over --rounds rounds, one child process per input, library and round.  PLAN lines: the interior share.
2. The in-process transport: P = 2 and 4 ranks on ONE GPU (tests/local_ranks.py: one thread per rank), halo_overlap = 1, mode 1, the
   community graph at --local-v vertices and Amazon's mean degree under contiguous blocks, and the uniform graph as the control; the
   switch off and on alternated over the rounds.  Per run: the median epoch time, and the timing families halo_deferred / halo_hidden
   summed over the ranks and the --epochs epochs.  The ranks share one GPU: a hidden exchange competes with the kernels for the same
   memory system -- a larger hidden share says the schedule works, it is no projected multi-GPU gain.
Then per line the median and the spread (min .. max) over the rounds, the ratio of the medians, and whether the medians differ by more
than the larger of the two spreads.  Every child runs under a time limit; the first that fails or runs out of time ends the run.
GPU box only:  python tools/gatmh_row_gather_overlap_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 300]"""
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
sys.path.insert(0, os.path.join(ROOT, "tests"))
DIMS, HEADS = [300, 128, 41], [8, 1]


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


def rate_child(graph, lib, path, calls):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import WORKLOADS
    from gatmh_row_gather_rate import gatmh_ctx
    V = WORKLOADS["amazon"][0]
    part = da.Partition.load(path)
    ctx, g = gatmh_ctx(da, part, DIMS, HEADS, V, 1, {})
    eng = da.NativeEngine(ctx)      # one epoch: every tensor the single passes below read is current
    eng.run(1)
    ctx.sync()
    eng.close()
    for arm in (("parent",) if lib == "parent" else ("off", "on")):
        if lib != "parent":
            ctx.gatmh_row_gather_overlap(1 if arm == "on" else 0)
            st = ctx.gatmh_row_gather_overlap_stats()
            N = int(g["localVtxCnt"])
            print("PLAN %s %s rows %d in_interior %d (%.4f) out_interior %d (%.4f)" %
                  (graph, arm, N, st["in_interior_rows"], st["in_interior_rows"] / N, st["out_interior_rows"], st["out_interior_rows"] / N))
        for layer in (1, 2):
            K = HEADS[layer - 1]
            zw = DIMS[layer] * (K if layer == 2 else 1)
            tag = "%s %s layer%d %dx%d" % (graph, arm, layer, K, zw // K)
            print("RATE %s forward ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.FORWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 1)
            ctx.aggregate(layer, da.BACKWARD)
            ctx.set_option("gatmh_bwd_phase", 2)
            print("RATE %s src ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 0)
        if lib != "parent":
            st = ctx.gatmh_row_gather_overlap_stats()
            print("PLAN %s %s passes split: forward %d source side %d" % (graph, arm, st["fwd_split"], st["src_split"]))
    ctx.close()


def local_child(graph, P, on, V, E, epochs):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import synth_edges
    from local_ranks import run_local
    src, dst = synth_edges("community" if graph == "community" else "uniform", V, E)
    parts = (np.arange(V, dtype=np.int64) * P // V).astype(np.int32)
    pobjs = [da.Partition.build(src, dst, parts, r, P) for r in range(P)]
    del src, dst
    kept = {}

    def setup(ctx, r, g):
        ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
        labels = np.random.default_rng(2).integers(0, DIMS[-1], V).astype(np.uint32)
        ctx.labels_upload(labels[g["localToGlobal"]])
        ctx.weights_init_xavier()
        ctx.gatmh_row_gather(1)
        ctx.gatmh_row_gather_overlap(on)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = (ctx.gatmh_row_gather_overlap_stats(), int(g["localVtxCnt"]))
            close()
        ctx.close = closing
    res = run_local(da, pobjs, parts, DIMS, da.GATMH, epochs, setup, {"gatmh_bwd_phase": 0, "halo_overlap": 1}, timing=True, warm_epochs=2,
                    pre=lambda c: c.gatmh_heads(HEADS), wnames=("w", "a_l", "a_r"))
    ms = float(np.median(np.max(np.stack([np.asarray(m, np.float64)[-epochs:] for m in res["epoch_ms"]]), axis=0)))
    tm = res["timing"]
    arm = "on" if on else "off"
    for r in sorted(kept):
        st, N = kept[r]
        print("PLAN local %s P%d %s rank %d rows %d in_interior %d out_interior %d fwd_split %d (%d in flight) src_split %d (%d in flight) deferred %d" %
              (graph, P, arm, r, N, st["in_interior_rows"], st["out_interior_rows"], st["fwd_split"], st["fwd_in_flight"], st["src_split"],
               st["src_in_flight"], st["bwd_deferred"]))
    print("LOCAL %s P%d %s epoch ms %.4f" % (graph, P, arm, ms))
    print("LOCAL %s P%d %s halo_deferred ms %.4f" % (graph, P, arm, tm["halo_deferred"]["ms"]))
    print("LOCAL %s P%d %s halo_hidden ms %.4f" % (graph, P, arm, tm["halo_hidden"]["ms"]))
    print("LOCAL %s P%d %s halo_waited ms %.4f" % (graph, P, arm, tm["halo_waited"]["ms"]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="a build of the parent commit (arm `parent`); without it that arm runs this tree's library")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--epochs", type=int, default=20)
    ap.add_argument("--local-v", type=int, default=400000)
    ap.add_argument("--step-timeout", type=int, default=300)
    ap.add_argument("--skip", default="", help="`compute` or `local`: leave that part out")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child and a.child[0] == "rate":
        rate_child(a.child[1], a.child[2], a.child[3], int(a.child[4]))
        return
    if a.child:
        local_child(a.child[1], int(a.child[2]), int(a.child[3]), int(a.child[4]), int(a.child[5]), int(a.child[6]))
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
            if ln.split(" ")[0] in ("RATE", "PLAN", "LOCAL"):
                say(ln)
        if r.returncode != 0:
            print("# step %s failed (%d): stopping\n%s" % (args, r.returncode, r.stderr[-2000:]), flush=True)
        return r.returncode == 0

    ok = True
    with tempfile.TemporaryDirectory() as tmp:
        V, E, _ = WORKLOADS["amazon"]
        paths = {}
        for graph in (() if a.skip == "compute" else ("community", "uniform")):
            t0 = time.time()
            parts = (np.arange(V, dtype=np.int64) * 8 // V).astype(np.int32)
            if graph == "community":
                src, dst = synth_edges("community", V, E)
                keep = (parts[src] == 0) | (parts[dst] == 0)          # the records rank 0 needs (the builder skips the others anyway)
                src, dst = src[keep], dst[keep]
            else:
                src, dst = synth_incident_edges(V, E, 0, 8)
            print("# %s: records of rank 0 generated, %.0f s" % (graph, time.time() - t0), flush=True)
            part = da.Partition.build(src, dst, parts, 0, 8)
            del src, dst, parts
            g = part.view()
            say("PART %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d" %
                (graph, int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"]), int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])))
            paths[graph] = os.path.join(tmp, graph + ".part")
            part.save(paths[graph])
            part.close()
            print("# %s: partition built and saved, %.0f s" % (graph, time.time() - t0), flush=True)
        for rnd in range(a.rounds):
            for graph in paths:
                for lib, so in (("parent", a.parent_lib), ("this", "")):
                    ok = ok and step(["rate", graph, lib, paths[graph], str(a.calls)], so)
            if not ok:
                break
    if ok and a.skip != "local":
        Vl = a.local_v
        El = int(Vl * (WORKLOADS["amazon"][1] / WORKLOADS["amazon"][0]))
        for rnd in range(a.rounds):
            for graph, P in (("community", 2), ("community", 4), ("uniform", 2)):
                for on in (0, 1):
                    ok = ok and step(["local", graph, str(P), str(on), str(Vl), str(El), str(a.epochs)], "")
            if not ok:
                break
    # per line: median and spread over the rounds
    med = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "RATE":
            med.setdefault(("RATE", w[1], w[3], w[4], w[5]), {}).setdefault(w[2], []).append(float(w[7]))     # graph, layer, shape, pass
        elif w[0] == "LOCAL":
            med.setdefault(("LOCAL", w[1], w[2], w[4], ""), {}).setdefault(w[3], []).append(float(w[6]))        # graph, P, quantity
    for key, arms in sorted(med.items()):
        base = "parent" if "parent" in arms else "off"
        p = arms[base]
        pm, ps = float(np.median(p)), max(p) - min(p)
        for arm in ("off", "on"):
            if arm not in arms or arm == base:
                continue
            x = arms[arm]
            xm, xs = float(np.median(x)), max(x) - min(x)
            verdict = "inside the spread" if abs(xm - pm) <= max(ps, xs) else "FASTER" if xm < pm else "NOT FASTER"
            if key[0] == "LOCAL" and key[3] != "epoch":
                verdict = ""
            say("RATIO %s arm %s over %s: %s %.4f (%.4f..%.4f) ms %.4f (%.4f..%.4f) ratio %.3f  %s" %
                (" ".join(k for k in key if k), arm, base, base, pm, min(p), max(p), xm, min(x), max(x), xm / pm if pm else float("nan"), verdict))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
