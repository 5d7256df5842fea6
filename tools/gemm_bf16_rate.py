#!/usr/bin/env python3
"""Does the bf16 matrix instruction pay in the vertex transforms (dory_gemm_bf16; csrc/gemm_bf16.hip), and what does fp32 parity cost on
it (dory_gemm_bf16_split; csrc/gemm_bf16_split.hip)?

Four arms, alternated over the rounds, every measurement a child process of its own under a time limit (the first that fails or runs
out of time ends the run):
  arm `parent`   --parent-lib (a build of the parent commit; without it the arm is left out)
  arm `off`      this tree's library, mode 0
  arm `bf16`     this tree's library, mode 2, the split off (K2b)
  arm `split`    this tree's library, mode 2, the split on (K2c)
PRODUCT lines: the device time (the library's `gemm` timing family, HIP events around K2's launches) of the three products of a
layer d_in -> d_out over V rows, on a GCN context whose graph is a ring (the vertex stage does not look at it):
  NN  forward of a hidden layer at layer 0 (z = ah W with the tanh epilogue)        TN  backward of layer 0 (dW = ah^T g)
  NT  backward of the same layer at layer 1 (TN, then grad = g W^T) minus the TN above
at  Reddit  V = 232 965: 602 -> 128, 128 -> 41     Amazon, one rank of 8  V = 1 178 761: 300 -> 64, 64 -> 64, 64 -> 25
    Friendster, 1 / 32 of its vertices  V = 2 050 261: 256 -> 48
FLOOR: the product's operand-plus-result bytes (dense: 4 (MK + KN + MN), the tanh output too in NN) at 5 TB/s, the copy rate
csrc/gemm.hip's notes use for the narrow products.
EPOCH lines: the Reddit-size GCN epoch (bench.py's uniform graph and loop) in the default order, transform-first
(gcn_transform_first = 2) and with the layer-0 aggregate kept (gcn_cache_ah0 = 1).
RATIO lines: medians with the runs' ranges; `inside the spread` when two medians differ by no more than the larger range.
GPU box only:  python tools/gemm_bf16_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 240] [--no-epochs] [--no-products]
               [--settings default,cached_ah0]"""
import argparse
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SHAPES = [("reddit", 232965, 602, 128), ("reddit", 232965, 128, 41), ("amazon/8", 1178761, 300, 64), ("amazon/8", 1178761, 64, 64),
          ("amazon/8", 1178761, 64, 25), ("friendster/32", 2050261, 256, 48)]
SETTINGS = {"default": {}, "transform_first": {"gcn_transform_first": 2}, "cached_ah0": {"gcn_cache_ah0": 1}}
ARMS = ("parent", "off", "bf16", "split")
CALLS = 10
COPY_TBPS = 5.0


def _timed(ctx, fn):
    fn()
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(CALLS):
        fn()
    ctx.sync()
    ms, n = ctx.timing_get("gemm")
    ctx.timing_enable(False)
    assert n
    return ms / CALLS


def _set_arm(ctx, arm):
    if arm in ("bf16", "split"):
        ctx.gemm_bf16(2)
    if arm == "split":
        ctx.gemm_bf16_split(1)


def product_child(arm, name, V, din, dout):
    import dorylus_amd as da
    V, din, dout = int(V), int(din), int(dout)
    ids = np.arange(V, dtype=np.uint32)
    part = da.Partition.build(ids, np.roll(ids, 1), np.zeros(V, np.int32), 0, 1)
    g = part.view()
    ms = {}
    for layer, dims in ((0, [din, dout, 2]), (1, [8, din, dout, 2])):
        ctx = da.Context(0)
        ctx.configure(da.GCN, dims, V, 0, 1)
        part.upload(ctx, None)
        ctx.preallocate()
        ctx.weights_init_xavier()
        _set_arm(ctx, arm)
        ctx.fill_uniform(layer, "ah", 1, -1.0, 1.0, g["localToGlobal"])
        ctx.fill_uniform(layer, "aTg", 2, -1.0, 1.0, g["localToGlobal"])
        fwd = _timed(ctx, lambda: ctx.apply_vertex(layer, da.FORWARD))
        bwd = _timed(ctx, lambda: ctx.apply_vertex(layer, da.BACKWARD))
        if layer == 0:
            ms["NN"], ms["TN"] = fwd, bwd
        else:
            ms["NT"] = bwd - ms["TN"]
        if arm != "parent":
            s = ctx.gemm_bf16_stats()
            assert (s["bf16_launches"] > 0) == (arm != "off") and s["fp32_while_on"] == 0, s
            assert ctx.gemm_bf16_split_stats()["split_launches"] == (s["bf16_launches"] if arm == "split" else 0)
        ctx.close()
    for form, (M, N, K) in (("NN", (V, dout, din)), ("NT", (V, din, dout)), ("TN", (din, dout, V))):
        floor = 4.0 * (M * K + K * N + M * N * (2 if form == "NN" else 1)) / (COPY_TBPS * 1e12) * 1e3
        print("PRODUCT %s V %d %d->%d %s %s ms %.4f floor_ms %.4f" % (name, V, din, dout, form, arm, ms[form], floor))


def epoch_child(arm, setting, path):
    import torch
    import dorylus_amd as da
    from bench import DIMS, REDDIT_V
    part = da.Partition.load(path)
    g = part.view()
    ctx = da.Context(0)
    ctx.configure(da.GCN, DIMS, REDDIT_V, 0, 1)
    part.upload(ctx, None)
    ctx.preallocate()
    for k, v in SETTINGS[setting].items():      # (after preallocate, as bench.py sets them)
        ctx.set_option(k, v)
    if setting == "transform_first" and not ctx.transform_first_active():
        print("# EPOCH reddit transform_first %s: the order is not active on this partition (asymmetric adjacency values): not measured" % arm)
        ctx.close()
        return
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
    print("EPOCH reddit %s %s ms %.4f gemm_ms %.4f" % (setting, arm, ms, ctx.timing_get("gemm")[0] / 20))
    eng.close()
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--no-epochs", action="store_true")
    ap.add_argument("--no-products", action="store_true")
    ap.add_argument("--settings", default=",".join(SETTINGS), help="the EPOCH lines to run")
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
            if ln.split(" ")[0] in ("PRODUCT", "EPOCH", "#"):
                say(ln)
        if r.returncode != 0:
            say("# step %s failed (%d): stopping\n%s" % (args, r.returncode, r.stderr[-2000:]))
        return r.returncode == 0

    arms = [x for x in ARMS if x != "parent" or a.parent_lib]
    steps = [["product", arm, name, str(V), str(din), str(dout)] for name, V, din, dout in SHAPES for arm in arms
             if not a.no_products]
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
            steps += [["epoch", arm, setting, path] for setting in a.settings.split(",") for arm in arms]
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
            med.setdefault(("PRODUCT " + " ".join(w[1:6]), w[10]), {}).setdefault(w[6], []).append(float(w[8]))
        elif w[0] == "EPOCH":
            med.setdefault(("EPOCH " + " ".join(w[1:3]), ""), {}).setdefault(w[3], []).append(float(w[5]))

    def verdict(x, y):
        mx, my = float(np.median(x)), float(np.median(y))
        spread = max(max(x) - min(x), max(y) - min(y))
        return "x%.3f %s" % (mx / my, "inside the spread" if abs(mx - my) <= spread else "FASTER" if mx < my else "NOT FASTER")
    for (key, floor), arms_ in sorted(med.items()):
        if "off" in arms_ and "bf16" in arms_:
            ln = "RATIO %s | " % key + " | ".join("%s_ms %.4f (%.4f..%.4f)" % (k, float(np.median(v)), min(v), max(v)) for k, v in arms_.items())
            ln += (" | floor_ms %s" % floor if floor else "") + " | bf16_over_off %s" % verdict(arms_["bf16"], arms_["off"])
            if "split" in arms_:
                ln += " | split_over_off %s | split_over_bf16 %s" % (verdict(arms_["split"], arms_["off"]), verdict(arms_["split"], arms_["bf16"]))
            if "parent" in arms_:
                ln += " | off_over_parent %s" % verdict(arms_["off"], arms_["parent"])
            say(ln)


if __name__ == "__main__":
    main()
