#!/usr/bin/env python3
"""What does walking every row's local entries before its ghost entries cost and hide (csrc/gat_mh_rows.hip,
dory_gatmh_row_gather_edge_split)?

1. Compute only, one rank, nothing in flight (as tools/gatmh_row_gather_overlap_rate.py runs it: rank 0 of 8, contiguous blocks, of an
   Amazon-size graph; the ghost tensors are filled once and never exchanged; dory_gatmh_row_gather(1); model 300-128-41, heads 8 / 1:
   rows of 128 floats on layer 1, of 64 floats on layer 2):
     community   bench.py's synth_edges("community"): 50 communities of consecutive ids, 85 % of the edges inside,
     uniform     bench.py's synth_incident_edges.
   fp32 rows, and bf16 rows (dory_gatmh_row_gather_bf16 + gatmh_bf16_gather = 2; dory_halo_bf16_ghosts / dory_gatmh_bf16_ghosts are
   set, but nothing is exchanged here, so the ghost rows are converted into the shadow rows by every pass of every arm alike).
   Per layer, the forward and the source side as single dory_aggregate calls (the library's timing family around the pass), and one
   compute epoch inside the engine, for
     parent   the library given with --parent-lib (a build of the parent commit),
     v0       this library, value 0,
     v1       this library, value 1: with nothing in flight ONE launch of the carry kernel over the local-first copy ("both"),
     v2       this library, value 2: two launches, the state of every boundary row written once and read once,
   the two libraries alternated over --rounds rounds, one child process per input, row format, library and round.
   PLAN lines: the local share of the entries and the boundary share of the rows.
2. The in-process transport: P = 2 and 4 ranks on ONE GPU (tests/local_ranks.py: one thread per rank), halo_overlap = 1, mode 1, the
   community graph at --local-v vertices and Amazon's mean degree under contiguous blocks: value 0, value 0 with
   dory_gatmh_row_gather_overlap, and value 1, alternated over the rounds.  Per run: the median epoch time, and the timing families
   halo_deferred / halo_hidden / halo_waited summed over the ranks and the --epochs epochs.  The ranks share one GPU: a hidden exchange
   competes with the kernels for the same memory system -- a larger hidden share says the schedule works, it is no projected
   multi-GPU gain.
Then per line the median and the spread (min .. max) over the rounds, the ratio of the medians, and whether the medians differ by more
than the larger of the two spreads.  Every child runs under a time limit; the first that fails or runs out of time ends the run.
GPU box only:  python tools/gatmh_row_gather_edge_split_rate.py [--out profiles/r31_gatmh_row_gather_edge_split.txt] [--parent-lib LIB]
               [--rounds 3] [--step-timeout 300]      (the file grows line by line: a run that is cut short leaves what it measured)"""
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
ARMS = {"v0": 0, "v1": 1, "v2": 2}


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


def rate_child(graph, fmt, lib, path, calls):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import WORKLOADS
    from gatmh_row_gather_rate import gatmh_ctx
    V = WORKLOADS["amazon"][0]
    part = da.Partition.load(path)
    ctx, g = gatmh_ctx(da, part, DIMS, HEADS, V, 1, {"gatmh_bf16_gather": 2} if fmt == "bf16" else {})
    if fmt == "bf16":
        ctx.gatmh_row_gather_bf16(1)
        ctx.halo_bf16_ghosts(1)
        ctx.gatmh_bf16_ghosts(1)
    eng = da.NativeEngine(ctx)      # one epoch: every tensor the single passes below read is current
    eng.run(1)
    ctx.sync()
    N = int(g["localVtxCnt"])
    for arm in (("parent",) if lib == "parent" else tuple(ARMS)):
        if lib != "parent":
            ctx.gatmh_row_gather_edge_split(ARMS[arm])
            if ARMS[arm]:
                st = ctx.gatmh_row_gather_edge_split_stats()
                nin, nout = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])
                bi = len(da.row_interior_plan(g["colPtr"], g["rowIdx"], N)[1])
                bo = len(da.row_interior_plan(g["rowPtr"], g["colIdx"], N)[1])
                print("PLAN %s %s %s rows %d in_entries %d local %d (%.4f) boundary_rows %d (%.4f) out_entries %d local %d (%.4f) boundary_rows %d (%.4f)" %
                      (graph, fmt, arm, N, nin, st["in_local_entries"], st["in_local_entries"] / max(1, nin), bi, bi / N,
                       nout, st["out_local_entries"], st["out_local_entries"] / max(1, nout), bo, bo / N))
        for layer in (1, 2):
            K = HEADS[layer - 1]
            zw = DIMS[layer] * (K if layer == 2 else 1)
            tag = "%s %s %s layer%d %dx%d" % (graph, fmt, arm, layer, K, zw // K)
            print("RATE %s forward ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.FORWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 1)
            ctx.aggregate(layer, da.BACKWARD)
            ctx.set_option("gatmh_bwd_phase", 2)
            print("RATE %s src ms %.4f" % (tag, timed(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD), calls)), flush=True)
            ctx.set_option("gatmh_bwd_phase", 0)
        ms = np.asarray(eng.run(calls + 1), np.float64)[1:]
        print("RATE %s %s %s epoch - compute ms %.4f" % (graph, fmt, arm, float(np.median(ms))), flush=True)
        if lib != "parent":
            st = ctx.gatmh_row_gather_edge_split_stats()
            print("PLAN %s %s %s passes that ran the carry kernels: forward %d source side %d" % (graph, fmt, arm, st["fwd_split"], st["src_split"]))
    eng.close()
    ctx.close()


def local_child(arm, P, V, E, epochs):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import synth_edges
    from local_ranks import run_local
    src, dst = synth_edges("community", V, E)
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
        ctx.gatmh_row_gather_overlap(1 if arm == "v0+overlap" else 0)
        ctx.gatmh_row_gather_edge_split(1 if arm == "v1" else 0)
        close = ctx.close

        def closing():
            if ctx.h:
                kept[r] = (ctx.gatmh_row_gather_edge_split_stats(), ctx.gatmh_row_gather_overlap_stats(), int(g["localVtxCnt"]))
            close()
        ctx.close = closing
    res = run_local(da, pobjs, parts, DIMS, da.GATMH, epochs, setup, {"gatmh_bwd_phase": 0, "halo_overlap": 1}, timing=True, warm_epochs=2,
                    pre=lambda c: c.gatmh_heads(HEADS), wnames=("w", "a_l", "a_r"))
    ms = float(np.median(np.max(np.stack([np.asarray(m, np.float64)[-epochs:] for m in res["epoch_ms"]]), axis=0)))
    tm = res["timing"]
    for r in sorted(kept):
        es, ov, N = kept[r]
        print("PLAN local P%d %s rank %d rows %d carry fwd %d (%d in flight) src %d (%d in flight) interior-row fwd %d (%d in flight) src %d (%d in flight) deferred %d" %
              (P, arm, r, N, es["fwd_split"], es["fwd_in_flight"], es["src_split"], es["src_in_flight"], ov["fwd_split"], ov["fwd_in_flight"],
               ov["src_split"], ov["src_in_flight"], ov["bwd_deferred"]))
    print("LOCAL community P%d %s epoch ms %.4f" % (P, arm, ms))
    for fam in ("halo_deferred", "halo_hidden", "halo_waited"):
        print("LOCAL community P%d %s %s ms %.4f" % (P, arm, fam, tm[fam]["ms"]))
    d = tm["halo_deferred"]["ms"]
    print("LOCAL community P%d %s hidden_share ms %.4f" % (P, arm, tm["halo_hidden"]["ms"] / d if d else 0.0), flush=True)


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
        rate_child(a.child[1], a.child[2], a.child[3], a.child[4], int(a.child[5]))
        return
    if a.child:
        local_child(a.child[1], int(a.child[2]), int(a.child[3]), int(a.child[4]), int(a.child[5]))
        return
    import dorylus_amd as da
    from bench import WORKLOADS, synth_edges, synth_incident_edges
    lines = []

    def say(ln):
        print(ln, flush=True)
        lines.append(ln)
        if a.out:                         # (kept as it grows: a run that is cut short leaves what it measured)
            with open(a.out, "a") as f:
                f.write(ln + "\n")

    if a.out:
        open(a.out, "w").close()

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
                for fmt in ("fp32", "bf16"):
                    for lib, so in (("parent", a.parent_lib), ("this", "")):
                        ok = ok and step(["rate", graph, fmt, lib, paths[graph], str(a.calls)], so)
            if not ok:
                break
    if ok and a.skip != "local":
        Vl = a.local_v
        El = int(Vl * (WORKLOADS["amazon"][1] / WORKLOADS["amazon"][0]))
        for rnd in range(a.rounds):
            for P in (2, 4):
                for arm in ("v0", "v0+overlap", "v1"):
                    ok = ok and step(["local", arm, str(P), str(Vl), str(El), str(a.epochs)], "")
            if not ok:
                break
    # per line: median and spread over the rounds
    med = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "RATE":
            med.setdefault(("RATE", w[1], w[2]) + tuple(w[4:-2]), {}).setdefault(w[3], []).append(float(w[-1]))     # graph, format, layer, shape, pass
        elif w[0] == "LOCAL":
            med.setdefault(("LOCAL", w[1], w[2], w[4]), {}).setdefault(w[3], []).append(float(w[6]))                # graph, P, quantity
    for key, arms in sorted(med.items()):
        pairs = [("v0", "parent"), ("v1", "v0"), ("v2", "v1")] if key[0] == "RATE" else [("v0+overlap", "v0"), ("v1", "v0"), ("v1", "v0+overlap")]
        for arm, base in pairs:
            if arm not in arms or base not in arms:
                continue
            p, x = arms[base], arms[arm]
            pm, ps = float(np.median(p)), max(p) - min(p)
            xm, xs = float(np.median(x)), max(x) - min(x)
            verdict = "inside the spread" if abs(xm - pm) <= max(ps, xs) else "FASTER" if xm < pm else "NOT FASTER"
            if key[0] == "LOCAL" and key[3] != "epoch":
                verdict = ""
            say("RATIO %s arm %s over %s: %s %.4f (%.4f..%.4f) %s %.4f (%.4f..%.4f) ratio %.3f  %s" %
                (" ".join(key), arm, base, base, pm, min(p), max(p), arm, xm, min(x), max(x), xm / pm if pm else float("nan"), verdict))
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
