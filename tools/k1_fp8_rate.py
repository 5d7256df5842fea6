#!/usr/bin/env python3
"""Do fp8 row gathers pay in K1, the row gather a partitioned rank of a large graph runs (dory_k1_fp8_gather)?

The setup of tools/k1_bf16_wide_rate.py: rank 0 of 8 as a GCN context of an 8-node run with its halo plans, spmm_variant = 0 (K1), the
ghost rows DELIVERED through dory_halo_unpack in both directions as fp32 wire rows (every arm: fp8 rows never travel, and the bf16
arm runs without twins so that both rounding arms convert their ghost rows); no peer and no link exist, the buffers are filled on the
device.
  input `uniform`   the Amazon-size uniform graph (bench.py's synth_incident_edges), rows of 300 (ld 320), 128 and 64 floats
  input `rmat`      the R-MAT graph of tools/gatmh_row_gather_hubs_rate.py (hub rows: the long-row kernels run), rows of 128 floats
  arm `parent`      --parent-lib (a build of the parent commit), fp32 rows
  arm `fp32`        this tree's library, mode 0
  arm `bf16`        this tree's library, gcn_bf16_gather = 2 (narrow)
  arm `fp8`         this tree's library, dory_k1_fp8_gather(2)
Per width the time of one dory_aggregate call, layer 1 forward (h@0, fg@1) and backward (grad@1, bg@0), everything included -- the
conversion of the local AND the ghost rows into the shadow rows, K1's launches: `ms` is a host clock around 10 calls back to back that
end in a device synchronise, after a warm call.  Beside it, from a second set of 10 calls under the library's timing families:
spmm_ms (K1's launches AND the ghost rows' conversion, which runs between them) and convert_ms (both conversions); gathered_TBps =
edges x row bytes over spmm_ms less the ghost rows' share of convert_ms (by rows).  The arms are
alternated over the rounds; every measurement is a child process of its own under a time limit; the first that fails or runs out of
time ends the run.  RATIO lines: medians, the runs' ranges, fp32 against parent (expected inside the spread), bf16 against fp32, fp8
against fp32 and fp8 against bf16; `inside the spread` when the medians differ by no more than the larger of the two arms' ranges.
TRAIN lines: the golden toy graph (tests/golden/parts_toy60_p1) trained for --train-epochs epochs with mode 0 and mode 2 from the same
weights: loss and accuracy sums of the first and the last epoch's forward pass.  KERNEL lines: the new kernels' vector registers.
GPU box only:  python tools/k1_fp8_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 120]"""
import argparse
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WIDTHS = {"uniform": (300, 128, 64), "rmat": (128,)}
ARMS = ("parent", "fp32", "bf16", "fp8")
ROW_BYTES = {"parent": 4, "fp32": 4, "bf16": 2, "fp8": 1}
CALLS = 10


def rate_child(graph, width, arm, path, parts_path):
    import torch
    import dorylus_amd as da
    from bench import WORKLOADS
    V = WORKLOADS["amazon"][0]
    W = int(width)
    part = da.Partition.load(path)
    parts = np.load(parts_path)
    g = part.view()
    N, Gs, Gd = int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
    nin, nout = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])
    ctx = da.Context(0)
    ctx.configure(da.GCN, [16, W, 8], V, 0, 8)
    ctx.set_option("spmm_variant", 0)
    ctx.set_option("gcn_bf16_gather", 2 if arm == "bf16" else 0)
    part.upload(ctx, parts)
    ctx.preallocate()
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
    ctx.fill_uniform(1, "grad", 2, -1.0, 1.0, g["localToGlobal"])
    if arm == "fp8":
        ctx.k1_fp8_gather(2)
    ld = (W + 31) // 32 * 32
    print("PART %s %d %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d" % (graph, W, arm, N, Gs, Gd, nin, nout))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    keep = []
    for direction, G in ((da.FORWARD, Gs), (da.BACKWARD, Gd)):
        eb, n = ctx.halo_wire_row(1, direction)
        assert (eb, n) == (4, ld), (eb, n, ld)
        rows = torch.rand((G, n), device="cuda", generator=gen) * 2 - 1
        rows[:, W:] = 0
        torch.cuda.synchronize()
        ctx.halo_unpack(1, direction, rows.data_ptr())
        keep.append(rows)
    ctx.sync()
    for direction, name, edges, G in ((da.FORWARD, "forward", nin, Gs), (da.BACKWARD, "backward", nout, Gd)):
        fn = lambda: ctx.aggregate(1, direction)
        fn()
        ctx.sync()
        t0 = time.perf_counter()
        for _ in range(CALLS):
            fn()
        ctx.sync()
        wall = (time.perf_counter() - t0) * 1e3 / CALLS
        ctx.timing_reset()
        ctx.timing_enable(True)
        for _ in range(CALLS):
            fn()
        ctx.sync()
        ms, n = ctx.timing_get("spmm")
        cv = ctx.timing_get("bf16_convert")[0] + (ctx.timing_get("fp8_convert")[0] if arm != "parent" else 0.0)
        ctx.timing_enable(False)
        assert n
        ms, cv = ms / CALLS, cv / CALLS
        local = cv * N / (N + G) if cv else 0.0      # (the conversion kernels are bound by the rows they read: split by rows)
        print("RATE %s %d %s ld %d %s ms %.4f spmm_ms %.4f convert_ms %.4f gathered_TBps %.3f" %
              (graph, W, arm, ld, name, wall, ms, cv, edges * ld * ROW_BYTES[arm] / (ms - (cv - local)) / 1e9))
    assert ctx.get_option("spmm_launches_k1") == 2 * (2 * CALLS + 1) and ctx.get_option("spmm_launches_k1s") == 0
    if arm != "parent":
        s = ctx.k1_fp8_gather_stats()
        print("STATS %s %d %s %s" % (graph, W, arm, " ".join("%s %d" % kv for kv in s.items())))
        assert s["fp8"] == (2 * (2 * CALLS + 1) if arm == "fp8" else 0) and s["other_family"] == s["no_form"] == 0, s
    ctx.close()


def train_child(mode, epochs):
    import dorylus_amd as da
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import partition_oracle as po
    d = os.path.join(ROOT, "tests", "golden", "parts_toy60_p1")
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
    for l in range(2):
        ctx.weight_set(l, "w", (rng.standard_normal((dims[l], dims[l + 1])) / np.sqrt(dims[l])).astype(np.float32))
    ctx.adam_config(0.01)
    ctx.k1_fp8_gather(int(mode))
    eng = da.NativeEngine(ctx)
    stat = []
    for _ in range(int(epochs)):
        eng.run(1)
        stat.append(ctx.train_stat())
    print("TRAIN toy60 dims 64-64-5 mode %s epochs %s first acc_sum %.1f loss_sum %.4f last acc_sum %.1f loss_sum %.4f rows %d fp8_aggregations %d" %
          (mode, epochs, stat[0][0], stat[0][1], stat[-1][0], stat[-1][1], stat[-1][2], ctx.k1_fp8_gather_stats()["fp8"]))
    eng.close()
    ctx.close()


def kernel_lines(this_lib):
    from gatmh_row_gather_bf16_wide_rate import kernel_notes
    return ["KERNEL %s vgprs %d spilled %d" % (name, vgpr, spill) for name, (vgpr, spill) in sorted(kernel_notes(this_lib).items()) if "fp8" in name]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="the library the parent arm runs on (a build of the parent commit); default: this tree's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--train-epochs", type=int, default=60)
    ap.add_argument("--graphs", nargs="*", default=list(WIDTHS))
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        (train_child if a.child[0] == "train" else rate_child)(*a.child[1:] if a.child[0] == "train" else a.child)
        return
    import dorylus_amd as da
    from bench import WORKLOADS, synth_edges, synth_incident_edges
    lines = []

    def say(ln):
        print(ln, flush=True)
        lines.append(ln)

    def flush_out():
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def step(args, lib):
        env = dict(os.environ)
        if lib:
            env["DORY_LIB_PATH"] = os.path.abspath(lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True,
                               timeout=a.step_timeout, env=env)
        except subprocess.TimeoutExpired:
            say("# step %s ran out of time: stopping" % (args[:3],))
            flush_out()
            return False
        for ln in r.stdout.splitlines():
            if ln.split(" ")[0] in ("RATE", "STATS", "PART", "TRAIN"):
                say(ln)
        if r.returncode != 0:
            say("# step %s failed (%d): stopping\n%s" % (args[:3], r.returncode, r.stderr[-2000:]))
        flush_out()
        return r.returncode == 0

    for ln in kernel_lines(da.LIB_PATH):
        say(ln)
    ok = all(step(["train", str(mode), str(a.train_epochs)], "") for mode in (0, 2))
    with tempfile.TemporaryDirectory() as tmp:
        V, E, _ = WORKLOADS["amazon"]
        parts = (np.arange(V, dtype=np.int64) * 8 // V).astype(np.int32)
        parts_path = os.path.join(tmp, "parts.npy")
        np.save(parts_path, parts)
        paths = {}
        for graph in a.graphs if ok else ():
            t0 = time.time()
            if graph == "rmat":
                src, dst = synth_edges("rmat", V, E)
                keep = (parts[src] == 0) | (parts[dst] == 0)          # the records rank 0 needs (the builder skips the others anyway)
                src, dst = src[keep], dst[keep]
            else:
                src, dst = synth_incident_edges(V, E, 0, 8)
            part = da.Partition.build(src, dst, parts, 0, 8)
            del src, dst
            paths[graph] = os.path.join(tmp, graph + ".part")
            part.save(paths[graph])
            part.close()
            print("# %s: partition built and saved, %.0f s" % (graph, time.time() - t0), flush=True)
        steps = [(graph, W, arm) for _ in range(a.rounds) for graph in a.graphs for W in WIDTHS[graph] for arm in ARMS]
        for graph, W, arm in steps:
            ok = ok and step([graph, str(W), arm, paths[graph], parts_path], a.parent_lib if arm == "parent" else "")
            if not ok:
                break
    # medians over the rounds with the runs' ranges
    med = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "RATE":
            med.setdefault((w[1], w[2], w[5], w[6]), {}).setdefault(w[3], []).append(float(w[8]))   # graph, width, ld, pass -> arm -> ms

    def verdict(x, y):           # arm x against arm y
        mx, my = float(np.median(x)), float(np.median(y))
        spread = max(max(x) - min(x), max(y) - min(y))
        return "x%.3f %s" % (mx / my, "inside the spread" if abs(mx - my) <= spread else "FASTER" if mx < my else "NOT FASTER")
    for key, arms in sorted(med.items()):
        if all(k in arms for k in ARMS):
            ln = "RATIO %s %s ld %s %s | " % key + " | ".join("%s_ms %.4f (%.4f..%.4f)" % (k, float(np.median(arms[k])), min(arms[k]), max(arms[k]))
                                                              for k in ARMS)
            ln += " | fp32_over_parent %s | bf16_over_fp32 %s | fp8_over_fp32 %s | fp8_over_bf16 %s" % (
                verdict(arms["fp32"], arms["parent"]), verdict(arms["bf16"], arms["fp32"]), verdict(arms["fp8"], arms["fp32"]),
                verdict(arms["fp8"], arms["bf16"]))
            say(ln)
    flush_out()


if __name__ == "__main__":
    main()
