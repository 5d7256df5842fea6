#!/usr/bin/env python
"""A/B of dory_gat_bf16_gather on the Reddit-size uniform GAT-prototype epoch that `bench.py --gnn gat` builds: one context,
one process, the modes alternated -- off, mode 2 narrow, mode 2 wide -- for three rounds, so that drift of the device shows up
as a difference between the rounds and not between the modes.  Per run: epoch ms (wall clock over the timed epochs), the
`spmm` timing family (ms per epoch and launches per epoch: K1s / K1 launches, combine and row_axpy kernels), `bf16_convert`
ms per epoch, the feature's counters, and each of the four aggregations called alone (`--reps` calls: ms per call of the
same two families).  One JSON line per run, then a summary line.

    python tools/gat_bf16_ab.py [--steps 10] [--warmup 3] [--rounds 3] [--scale 1.0] [--opt key=value ...]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONFIGS = [("off", 0, 0), ("mode2_narrow", 2, 0), ("mode2_wide", 2, 1)]
FAMILIES = ("spmm", "bf16_convert", "gemm", "edge", "loss", "adam")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=10, help="calls per aggregation of the per-aggregation timings")
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the Reddit edge count")
    ap.add_argument("--opt", action="append", default=[], help="key=value for set_option, before the graph is uploaded")
    args = ap.parse_args()
    import torch
    import bench
    import dorylus_amd as da
    torch.cuda.set_device(0)
    V, E_full, dims = bench.WORKLOADS["reddit"]
    src, dst = bench.synth_edges("uniform", V, int(E_full * args.scale))
    part = da.Partition.build(src, dst, np.zeros(V, np.int32), 0, 1)
    del src, dst
    g = part.view()
    ctx = da.Context(0)
    ctx.configure(da.GAT, dims, V, 0, 1)
    for kv in args.opt:
        k, v = kv.split("=")
        ctx.set_option(k, int(v))
    part.upload(ctx, None)
    ctx.preallocate()
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
    labels = np.random.default_rng(2).integers(0, dims[-1], V).astype(np.uint32)
    ctx.labels_upload(labels[g["localToGlobal"]])
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    eng = da.NativeEngine(ctx)
    runs = []
    for rnd in range(args.rounds):
        for name, mode, wide in CONFIGS:
            ctx.gat_bf16_gather(mode, wide)
            ctx.timing_enable(False)
            eng.run(args.warmup)
            ctx.timing_reset()
            ctx.timing_enable(True)
            s0 = ctx.gat_bf16_gather_stats()
            l0 = [ctx.get_option(k) for k in ("spmm_launches_k1s", "spmm_launches_k1b", "spmm_launches_k1")]
            ctx.sync()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            eng.run(args.steps)
            ctx.sync()
            torch.cuda.synchronize()
            ms = (time.perf_counter() - t0) * 1e3 / args.steps
            fam = {f: ctx.timing_get(f) for f in FAMILIES}
            s1 = ctx.gat_bf16_gather_stats()
            l1 = [ctx.get_option(k) for k in ("spmm_launches_k1s", "spmm_launches_k1b", "spmm_launches_k1")]
            r = {"round": rnd, "config": name, "mode": mode, "wide": wide, "epoch_ms": round(ms, 4),
                 "ms_per_epoch": {f: round(v[0] / args.steps, 4) for f, v in fam.items() if v[1]},
                 "timed_intervals_per_epoch": {f: v[1] / args.steps for f, v in fam.items() if v[1]},
                 "bf16_aggregations_per_epoch": {k: (s1[k] - s0[k]) / args.steps for k in s1},
                 "aggregations_per_epoch_k1s_k1b_k1": [(b - a) / args.steps for a, b in zip(l0, l1)],
                 "epoch_graph_recorded": int(ctx.get_option("epoch_graph_recorded")),
                 "gate_timeouts": int(ctx.get_option("spmm_gate_timeouts"))}
            # the four aggregations one by one on the tensors the last epoch left (dory_aggregate alone, `reps` calls each; a
            # forward one follows its layer's edge forward and a backward one its layer's forward, so arow and gat_reuse_nsum's
            # kept sum are current and the calls take the epoch's paths): ms per call of the spmm family
            # (the K1s launches, the combine and row_axpy kernels) and of the conversions
            per = {}
            for layer in range(1, len(dims)):
                for dname, d in (("fwd", da.FORWARD), ("bwd", da.BACKWARD)):
                    if d == da.FORWARD:      # "A" holds one layer's scores at a time: this layer's edge forward again, as in the epoch
                        ctx.apply_edge(layer, da.FORWARD)
                    ctx.aggregate(layer, d)
                    ctx.timing_reset()
                    for _ in range(args.reps):
                        ctx.aggregate(layer, d)
                    ctx.sync()
                    per[f"{dname}{layer}_F{dims[layer]}"] = {f: round(ctx.timing_get(f)[0] / args.reps, 4) for f in ("spmm", "bf16_convert")
                                                            if ctx.timing_get(f)[1]}
            r["ms_per_aggregation"] = per
            runs.append(r)
            print(json.dumps(r), flush=True)
    summary = {}
    for name, _, _ in CONFIGS:
        mine = [r for r in runs if r["config"] == name]
        ep = [r["epoch_ms"] for r in mine]
        summary[name] = {"epoch_ms_rounds": ep, "epoch_ms_min": min(ep), "epoch_ms_max": max(ep),
                         "spmm_ms_rounds": [r["ms_per_epoch"].get("spmm") for r in mine],
                         "bf16_convert_ms_rounds": [r["ms_per_epoch"].get("bf16_convert", 0.0) for r in mine],
                         "spmm_ms_per_aggregation_rounds": {k: [r["ms_per_aggregation"][k].get("spmm") for r in mine] for k in mine[0]["ms_per_aggregation"]}}
    print(json.dumps({"summary": summary, "steps": args.steps, "warmup": args.warmup, "V": int(V), "in_edges": int(g["localInEdgeCnt"]),
                      "dims": list(dims), "stats_total": ctx.gat_bf16_gather_stats()}), flush=True)
    eng.close()
    ctx.close()


if __name__ == "__main__":
    main()
