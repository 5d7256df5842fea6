#!/usr/bin/env python3
"""What do bf16 rows buy the multi-head GAT's row-gather kernels (csrc/gat_mh_rows.hip, dory_gatmh_row_gather_bf16)?

  1. Rank 0 of 8 of the Amazon-size uniform graph, as tools/gatmh_row_gather_rate.py builds and runs it (compute only: the ghost
     tensors are filled once and never exchanged), mode 1.  Two models: 300-128-41 with heads 8 / 1 (8 x 16 = 128-float rows, then
     1 x 41 = 64-float rows; both destination sides are the row-wise kernel) and 300-64-25 with heads 32 / 1 (32 x 2 = 64-float rows,
     then 1 x 25 = 32-float rows; both destination sides are the edge pass).  Per layer and pass the device time of single
     dory_aggregate calls (the library's timing family around the pass: the bf16 arm's figure INCLUDES the conversion of the rows
     into the shadow buffer, which is also given alone) and TB/s of gathered rows = edges x row bytes / time.
     Arm `fp32`: gatmh_bf16_gather = 0 (any library); arm `bf16`: dory_gatmh_row_gather_bf16(1), gatmh_bf16_gather = 2.
     With --fp32-lib the fp32 arm runs on that library (a build of the parent commit), the two alternated over --rounds rounds.
  2. The size of the known consequence (include/dorylus_hip.h): one epoch at the same weights on a 20 000-vertex graph, single
     partition, 40-128-41 heads 8 / 1 -- the largest deviation of dz, del and the a_l / a_r gradients of gatmh_bf16_gather = 2 from the
     fp32 run of the same family, relative to the fp32 run's largest magnitude; once for the row-gather family (mode 1) and once for
     the sweep forms (mode 0, spmm_blk_nb = 8) on the same inputs.
Every measurement is a child process of its own under a time limit; the first that fails or runs out of time ends the run.
GPU box only:  python tools/gatmh_row_gather_bf16_rate.py [--out FILE] [--fp32-lib LIB] [--rounds 3] [--step-timeout 240]"""
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


def timed2(ctx, fam, fn, calls=10):
    """(ms per call of family `fam`, of that the conversion into the shadow rows)"""
    fn()
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(calls):
        fn()
    ctx.sync()
    ms, n = ctx.timing_get(fam)
    cv, _ = ctx.timing_get("bf16_convert")
    ctx.timing_enable(False)
    assert n, fam
    return ms / calls, cv / calls


def rate_child(model, arm, path):
    import torch  # noqa: F401
    import dorylus_amd as da
    from bench import WORKLOADS
    from gatmh_row_gather_rate import epoch_ms, gatmh_ctx
    V = WORKLOADS["amazon"][0]
    part = da.Partition.load(path)
    dims, heads = MODELS[model]
    ctx, g = gatmh_ctx(da, part, dims, heads, V, 1, {})
    nin, nout = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])
    bf = arm == "bf16"
    if bf:
        ctx.gatmh_row_gather_bf16(1)
        ctx.set_option("gatmh_bf16_gather", 2)
    print("EPOCH %s %s ms %.3f" % (model, arm, epoch_ms(ctx, da)))
    for layer in (1, 2):
        K = heads[layer - 1]
        zw = dims[layer] * (K if layer == 2 else 1)
        ld = (zw + 31) // 32 * 32
        rb = ld * (2 if bf else 4)
        tag = "%s %s layer%d %dx%d ld %d" % (model, arm, layer, K, zw // K, ld)
        before = ctx.gatmh_row_gather_stats()
        fwd, cv = timed2(ctx, "spmm", lambda: ctx.aggregate(layer, da.FORWARD))
        print("RATE %s forward ms %.4f convert_ms %.4f gathered_TBps %.3f" % (tag, fwd, cv, nin * rb / fwd / 1e9))
        ctx.set_option("gatmh_bwd_phase", 1)
        ctx.aggregate(layer, da.BACKWARD)
        d = [a - b for a, b in zip(ctx.gatmh_row_gather_stats(), before)]
        if d[1] > 0:
            dst, cv = timed2(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD))
            print("RATE %s dst_edge_pass ms %.4f convert_ms %.4f gathered_TBps %.3f" % (tag, dst, cv, nin * rb / dst / 1e9))
        ctx.set_option("gatmh_bwd_phase", 2)
        src, cv = timed2(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD))
        ctx.set_option("gatmh_bwd_phase", 0)
        print("RATE %s src ms %.4f convert_ms %.4f gathered_TBps %.3f" % (tag, src, cv, nout * rb / src / 1e9))
    if bf:
        st = ctx.gatmh_row_gather_bf16_stats()
        assert st[0] > 0 and st[2] > 0, st
    ctx.close()


def deviation_child():
    import torch  # noqa: F401
    import dorylus_amd as da
    dims, heads, V = [40, 128, 41], [8, 1], 20000
    rng = np.random.default_rng(11)
    s, d = rng.integers(0, V, 13 * V).astype(np.uint32), rng.integers(0, V, 13 * V).astype(np.uint32)
    part = da.Partition.build(s, d, np.zeros(V, np.int32), 0, 1)
    X = rng.uniform(-1, 1, (V, dims[0])).astype(np.float32)
    y = rng.integers(0, dims[-1], V).astype(np.uint32)
    params = []
    for l in range(2):
        zw = dims[l + 1]
        params.append([(rng.standard_normal((dims[l], zw)) / np.sqrt(dims[l])).astype(np.float32),
                       (rng.standard_normal(zw) * 0.3).astype(np.float32), (rng.standard_normal(zw) * 0.3).astype(np.float32)])

    def run(rows, v):
        ctx = da.Context(0)
        ctx.configure(da.GATMH, dims, V)
        ctx.gatmh_heads(heads)
        ctx.set_option("spmm_blk_nb", 8)
        part.upload(ctx, None)
        ctx.preallocate()
        ctx.upload(0, "h", X)
        ctx.labels_upload(y)
        for l, (W, al, ar) in enumerate(params):
            ctx.weight_set(l, "w", W); ctx.weight_set(l, "a_l", al); ctx.weight_set(l, "a_r", ar)
        ctx.adam_config(0.01)
        ctx.gatmh_row_gather(1 if rows else 0)
        if rows:
            ctx.gatmh_row_gather_bf16(1)
        ctx.set_option("gatmh_bf16_gather", v)
        eng = da.NativeEngine(ctx)
        eng.run(1)
        out = {}
        for l in range(2):
            out[(l, "dz")], out[(l, "del")] = ctx.download(l, "dz"), ctx.download(l, "del")
            out[(l, "g_a_l")], out[(l, "g_a_r")] = ctx.weight_grad_get(l, "a_l"), ctx.weight_grad_get(l, "a_r")
        passes = (ctx.gatmh_row_gather_stats(), ctx.get_option("gatmh_bf16_gathers_fwd"), ctx.get_option("gatmh_bf16_gathers_src"))
        eng.close()
        ctx.close()
        return out, passes
    for fam, rows in (("row_gather", True), ("sweep", False)):
        ref, p0 = run(rows, 0)
        got, p2 = run(rows, 2)
        assert (p2[0][0] > 0) == rows and p2[1] == 2 and p2[2] == 2 and p0[1] == 0, (fam, p0, p2)
        for k in sorted(ref):
            a, b = ref[k].astype(np.float64), got[k].astype(np.float64)
            print("DEVIATION %s layer %d %s max_abs_dev_over_max_abs %.3e" % (fam, k[0], k[1], np.abs(a - b).max() / np.abs(a).max()))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--fp32-lib", default="", help="the library the fp32 arm runs on (a build of the parent commit); default: this tree's")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        if a.child[0] == "deviation":
            deviation_child()
        else:
            rate_child(*a.child)
        return
    import dorylus_amd as da
    from bench import WORKLOADS, synth_incident_edges
    lines = []

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
        got = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("RATE", "EPOCH", "DEVIATION")]
        for ln in got:
            print(ln, flush=True)
        lines.extend(got)
        if r.returncode != 0:
            print("# step %s failed (%d): stopping\n%s" % (args, r.returncode, r.stderr[-2000:]), flush=True)
        return r.returncode == 0

    with tempfile.TemporaryDirectory() as tmp:
        V, E, _ = WORKLOADS["amazon"]
        src, dst = synth_incident_edges(V, E, 0, 8)
        parts = (np.arange(V, dtype=np.int64) * 8 // V).astype(np.int32)
        part = da.Partition.build(src, dst, parts, 0, 8)
        del src, dst
        path = os.path.join(tmp, "amazon.part")
        part.save(path)
        part.close()
        ok = True
        for rnd in range(a.rounds):
            for model in MODELS:
                for arm, lib in (("fp32", a.fp32_lib), ("bf16", "")):
                    ok = ok and step([model, arm, path], lib)
                    if not ok:
                        break
                if not ok:
                    break
            if not ok:
                break
        if ok:
            step(["deviation"], "")
    # medians over the rounds, and bf16 (conversion included) against fp32
    med = {}
    for ln in lines:
        if ln.startswith("RATE "):
            w = ln.split()
            key = (w[1], w[3], w[4], w[6], w[7])                  # model, layer, shape, ld, pass
            med.setdefault(key, {}).setdefault(w[2], []).append(float(w[9]))
    for key, arms in sorted(med.items()):
        if "fp32" in arms and "bf16" in arms:
            f, b = float(np.median(arms["fp32"])), float(np.median(arms["bf16"]))
            out = "RATIO %s %s %s ld %s %s fp32_ms %.4f bf16_ms %.4f bf16_over_fp32 %.3f%s" % (
                key + (f, b, b / f, "" if b < f else "  (NOT FASTER)"))
            print(out, flush=True)
            lines.append(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
