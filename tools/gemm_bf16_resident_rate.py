#!/usr/bin/env python3
"""Does a resident bf16 A operand pay in the layer-0 products of K2b (dory_gemm_bf16_resident; csrc/gemm_bf16_resident.hip)?

Arms, alternated over the rounds, every measurement a child process of its own under a time limit (the first that fails or runs out
of time ends the run):
  arm `parent`   --parent-lib (a build of the parent commit, dory_gemm_bf16 mode 2; without it the arm is left out)
  arm `off`      this tree's library, mode 2, the switch off (K2b)
  arm `on`       this tree's library, mode 2, the switch on (K2r)
PRODUCT lines: the device time (the library's `gemm` timing family) of the two layer-0 products of a GCN hidden layer d_in -> d_out
over V rows on a ring with gcn_cache_ah0 = 1, the aggregate made once and kept: NN z = ah@0 W with the tanh epilogue, TN dW = ah@0^T g
-- the layer-0 operand forced at every shape.  CONVERT lines: the one-off conversion (`bf16_convert` family), timed once.
FLOOR: the bytes of the product (the tanh output too in NN) at 5 TB/s with the A operand at 4 (parent, off) or 2 (on) bytes an element.
EPOCH lines: the Reddit-size GCN epoch (bench.py's uniform graph and loop) with the layer-0 aggregate kept (gcn_cache_ah0 = 1).
RATIO lines: medians with the runs' ranges; `inside the spread` when two medians differ by no more than the larger range.
GPU box only:  python tools/gemm_bf16_resident_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 240] [--no-epochs]"""
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
SHAPES = [("reddit", 232965, 602, 128), ("reddit", 232965, 128, 41), ("amazon/8", 1178761, 300, 64), ("friendster/32", 2050261, 256, 48)]
ARMS = ("parent", "off", "on")
COPY_TBPS = 5.0


def _set_arm(ctx, arm):
    ctx.gemm_bf16(2)
    if arm == "on":
        ctx.gemm_bf16_resident(1)


def product_child(arm, name, V, din, dout):
    import dorylus_amd as da
    from gemm_bf16_rate import CALLS, _timed
    V, din, dout = int(V), int(din), int(dout)
    ids = np.arange(V, dtype=np.uint32)
    part = da.Partition.build(ids, np.roll(ids, 1), np.zeros(V, np.int32), 0, 1)
    g = part.view()
    ctx = da.Context(0)
    ctx.configure(da.GCN, [din, dout, 2], V, 0, 1)
    part.upload(ctx, None)
    ctx.preallocate()
    ctx.set_option("gcn_cache_ah0", 1)
    ctx.weights_init_xavier()
    _set_arm(ctx, arm)
    ctx.fill_uniform(0, "x", 1, -1.0, 1.0, g["localToGlobal"])
    ctx.fill_uniform(0, "aTg", 2, -1.0, 1.0, g["localToGlobal"])
    ctx.aggregate(0, da.FORWARD)      # ah@0, kept from here on: the A operand of both products
    if arm == "on":      # the one-off conversion, outside the product's time
        ctx.timing_reset()
        ctx.timing_enable(True)
        ctx.apply_vertex(0, da.FORWARD)
        ctx.sync()
        print("CONVERT %s V %d %d->%d ms %.4f" % (name, V, din, dout, ctx.timing_get("bf16_convert")[0]))
        ctx.timing_enable(False)
    ms = {"NN": _timed(ctx, lambda: ctx.apply_vertex(0, da.FORWARD)), "TN": _timed(ctx, lambda: ctx.apply_vertex(0, da.BACKWARD))}
    if arm == "on":
        s = ctx.gemm_bf16_resident_stats()
        assert s["conversions"] == 1 and s["plain_while_on"] == 0 and s["resident_launches"] == 2 * (CALLS + 1) + 1, s
    ctx.close()
    ab = 2.0 if arm == "on" else 4.0
    for form, (M, N, K) in (("NN", (V, dout, din)), ("TN", (din, dout, V))):
        floor = (ab * M * K + 4.0 * (K * N + M * N * (2 if form == "NN" else 1))) / (COPY_TBPS * 1e12) * 1e3
        print("PRODUCT %s V %d %d->%d %s %s ms %.4f floor_ms %.4f" % (name, V, din, dout, form, arm, ms[form], floor))


def epoch_child(arm, path):
    import torch
    import dorylus_amd as da
    from bench import DIMS, REDDIT_V
    part = da.Partition.load(path)
    g = part.view()
    ctx = da.Context(0)
    ctx.configure(da.GCN, DIMS, REDDIT_V, 0, 1)
    part.upload(ctx, None)
    ctx.preallocate()
    ctx.set_option("gcn_cache_ah0", 1)
    _set_arm(ctx, arm)
    ctx.fill_uniform(0, "x", 1, -1.0, 1.0, g["localToGlobal"])
    ctx.labels_upload(np.random.default_rng(2).integers(0, DIMS[-1], REDDIT_V).astype(np.uint32)[g["localToGlobal"]])
    ctx.weights_init_xavier()
    ctx.adam_config(0.01)
    eng = da.NativeEngine(ctx)
    eng.run(3)
    ctx.timing_reset()
    ctx.timing_enable(True)
    ctx.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    eng.run(20)
    ctx.sync()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) * 1e3 / 20
    note = " stats %s" % ctx.gemm_bf16_resident_stats() if arm == "on" else ""
    print("EPOCH reddit cached_ah0 %s ms %.4f gemm_ms %.4f%s" % (arm, ms, ctx.timing_get("gemm")[0] / 20, note))
    eng.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--no-epochs", action="store_true")
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        (product_child if a.child[0] == "product" else epoch_child)(*a.child[1:])
        return
    lines = []

    def say(ln):
        print(ln, flush=True)
        lines.append(ln)
        if a.out:
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")

    def step(args, arm):
        env = dict(os.environ)
        if arm == "parent":
            env["DORY_LIB_PATH"] = os.path.abspath(a.parent_lib)
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child"] + args, capture_output=True, text=True,
                               timeout=a.step_timeout, env=env)
        except subprocess.TimeoutExpired:
            say("# step %s ran out of time: stopping" % (args,))
            return False
        for ln in r.stdout.splitlines():
            if ln.split(" ")[0] in ("PRODUCT", "EPOCH", "CONVERT", "#"):
                say(ln)
        if r.returncode != 0:
            say("# step %s failed (%d): stopping\n%s" % (args, r.returncode, r.stderr[-2000:]))
        return r.returncode == 0

    arms = [x for x in ARMS if x != "parent" or a.parent_lib]
    steps = [["product", arm, name, str(V), str(din), str(dout)] for name, V, din, dout in SHAPES for arm in arms]
    with tempfile.TemporaryDirectory() as tmp:
        if not a.no_epochs:
            import dorylus_amd as da
            from bench import REDDIT_E, REDDIT_V, synth_edges
            src, dst = synth_edges("uniform", REDDIT_V, REDDIT_E)
            part = da.Partition.build(src, dst, np.zeros(REDDIT_V, np.int32), 0, 1)
            del src, dst
            path = os.path.join(tmp, "reddit.part")
            part.save(path)
            part.close()
            steps += [["epoch", arm, path] for arm in arms]
        ok = True
        for rnd in range(a.rounds):
            for s in steps:
                ok = ok and step(s, s[1])
                if not ok:
                    break
            if not ok:
                break
    med = {}
    for ln in lines:
        w = ln.split() or [""]
        if w[0] == "PRODUCT":
            med.setdefault("PRODUCT " + " ".join(w[1:6]), {}).setdefault(w[6], []).append(float(w[8]))
        elif w[0] == "EPOCH":
            med.setdefault("EPOCH " + " ".join(w[1:3]), {}).setdefault(w[3], []).append(float(w[5]))

    def verdict(x, y):
        mx, my = float(np.median(x)), float(np.median(y))
        spread = max(max(x) - min(x), max(y) - min(y))
        return "x%.3f %s" % (mx / my, "inside the spread" if abs(mx - my) <= spread else "FASTER" if mx < my else "NOT FASTER")
    for key, arms_ in sorted(med.items()):
        if "off" in arms_ and "on" in arms_:
            ln = "RATIO %s | " % key + " | ".join("%s_ms %.4f (%.4f..%.4f)" % (k, float(np.median(v)), min(v), max(v)) for k, v in arms_.items())
            ln += " | on_over_off %s" % verdict(arms_["on"], arms_["off"])
            if "parent" in arms_:
                ln += " | on_over_parent %s | off_over_parent %s" % (verdict(arms_["on"], arms_["parent"]), verdict(arms_["off"], arms_["parent"]))
            say(ln)


if __name__ == "__main__":
    main()
