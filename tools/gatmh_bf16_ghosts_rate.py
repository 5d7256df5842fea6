#!/usr/bin/env python3
"""Do the bf16 row gathers of the multi-head GAT's row-gather kernels pay once the ghost rows arrive as bf16 and stay
(dory_gatmh_bf16_ghosts: twins for fg_z / bg_do)?

Rank 0 of 8 of the Amazon-size uniform graph as tools/gatmh_row_gather_bf16_rate.py builds it, but as a context of an 8-node run with
its halo plans: the ghost rows are DELIVERED through the split entry points -- z -> fg_z by dory_halo_unpack from a buffer of bf16 wire
rows, do / st -> bg_do / bg_st by dory_gatmh_bwd_unpack from a buffer of merged rows -- so that the twin is what lands.  No peer and no
link exist: the buffers are filled on the device.  Mode 1 (the family in place of every other form), gatmh_bwd_phase 1 / 2.
  arm `fp32`    gatmh_bf16_gather = 0, ghost tensors filled once (fp32 rows)                                   -- the comparison r26 lost
  arm `parent`  --parent-lib (a build of the parent commit; default: this tree's with the new switch off): dory_halo_bf16_rows +
                dory_gatmh_halo_bf16 + dory_halo_bf16_ghosts, gatmh_bf16_gather = 2: the rows arrive as bf16, are widened into the fp32
                ghost tensor and every bf16 pass converts N + ghosts rows                                      -- r26's "conversion included"
  arm `twins`   this tree's library with dory_gatmh_bf16_ghosts on top: every bf16 pass converts its N local rows and gathers the ghost
                rows from the twin
Per layer and pass the device time of single dory_aggregate calls (the library's timing family around the pass, the conversion that
belongs to it INCLUDED and also given alone), the unpacks (timing family "halo") and dory_apply_edge ("edge": the scores of the ghost
rows from fp32 rows / from the twin), and a compute epoch driven call by call (forward of both layers, predict, both backward phases of
both layers, the weight gradients; no exchange, no Adam), wall clock.
Every measurement is a child process of its own under a time limit; the first that fails or runs out of time ends the run.
GPU box only:  python tools/gatmh_bf16_ghosts_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 240]"""
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
# rows of 128 / 64, 64 / 32 and 64 / 32 floats; heads 8 x 16, 8 x 8, 32 x 2 (the last layer: one head)
MODELS = {"8x16": ([300, 128, 41], [8, 1]), "8x8": ([300, 64, 25], [8, 1]), "32x2": ([300, 64, 25], [32, 1])}
ARMS = ("fp32", "parent", "twins")
WARM, STEPS = 2, 5


def rate_child(model, arm, path, parts_path):
    import torch
    import dorylus_amd as da
    from bench import WORKLOADS
    from gatmh_row_gather_bf16_rate import timed2
    V = WORKLOADS["amazon"][0]
    part = da.Partition.load(path)
    parts = np.load(parts_path)
    dims, heads = MODELS[model]
    g = part.view()
    N, Gs, Gd = int(g["localVtxCnt"]), int(g["srcGhostCnt"]), int(g["dstGhostCnt"])
    nin, nout = int(g["localInEdgeCnt"]), int(g["localOutEdgeCnt"])
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, V, 0, 8)
    ctx.gatmh_heads(heads)
    ctx.gatmh_row_gather(1)
    part.upload(ctx, parts)
    ctx.preallocate()
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
    labels = np.random.default_rng(2).integers(0, dims[-1], V).astype(np.uint32)
    ctx.labels_upload(labels[g["localToGlobal"]])
    ctx.weights_init_xavier()
    bf = arm != "fp32"
    if bf:
        ctx.gatmh_row_gather_bf16(1)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.halo_bf16_rows(1)
        ctx.gatmh_halo_bf16(1)
        ctx.halo_bf16_ghosts(1)
        if arm == "twins":
            ctx.gatmh_bf16_ghosts(1)
    print("PART %s %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d" % (model, arm, N, Gs, Gd, nin, nout))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    deliver = {}
    for layer in (1, 2):
        l, K = layer - 1, heads[layer - 1]
        zw = dims[layer] * (K if layer == 2 else 1)
        ld = (zw + 31) // 32 * 32
        tag = "%s %s layer%d %dx%d ld %d" % (model, arm, layer, K, zw // K, ld)
        if not bf:            # fp32 rows, filled once
            ctx.fill_uniform(l, "fg_z", 2 + l, -1.0, 1.0)
            ctx.fill_uniform(l, "bg_do", 6 + l, -1.0, 1.0)
            ctx.fill_uniform(l, "bg_st", 8 + l, 0.25, 1.0)
            deliver[layer] = (lambda: None, lambda: None)
            continue
        eb, n = ctx.halo_wire_row(layer, da.FORWARD)
        assert (eb, n) == (2, ld), (eb, n, ld)
        z16 = (torch.rand((Gs, ld), device="cuda", generator=gen) * 2 - 1).to(torch.bfloat16)
        z16[:, zw:] = 0
        R, dof, k4 = ctx.gatmh_bwd_wire_row(l)
        assert ctx.gatmh_bwd_wire_do(l) == (2, ld) and dof == ld // 2 and k4 == 4 * K
        rows = torch.rand((Gd, R), device="cuda", generator=gen) * 0.75 + 0.25
        do16 = (torch.rand((Gd, ld), device="cuda", generator=gen) * 2 - 1).to(torch.bfloat16)
        do16[:, zw:] = 0
        rows[:, :dof] = do16.view(torch.float32)
        del do16
        torch.cuda.synchronize()
        fwd = (lambda layer=layer, z16=z16: ctx.halo_unpack(layer, da.FORWARD, z16.data_ptr()))
        bwd = (lambda l=l, rows=rows: ctx.gatmh_bwd_unpack(l, rows.data_ptr()))
        deliver[layer] = (fwd, bwd)
        ms, _ = timed2(ctx, "halo", fwd)
        print("UNPACK %s fg_z ms %.4f" % (tag, ms))
        ms, _ = timed2(ctx, "halo", bwd)
        print("UNPACK %s bg_do_st ms %.4f" % (tag, ms))

    def epoch():
        for layer in (1, 2):
            ctx.apply_vertex(layer - 1, da.FORWARD)
            ctx.apply_edge(layer, da.FORWARD)
            ctx.aggregate(layer, da.FORWARD)
        ctx.predict_gat(2)
        for layer in (2, 1):
            ctx.set_option("gatmh_bwd_phase", 1)
            ctx.aggregate(layer, da.BACKWARD)
            ctx.set_option("gatmh_bwd_phase", 2)
            ctx.aggregate(layer, da.BACKWARD)
            ctx.apply_vertex(layer - 1, da.BACKWARD)
        ctx.set_option("gatmh_bwd_phase", 0)
    for _ in range(WARM):
        epoch()
    ctx.sync()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(STEPS):
        epoch()
    ctx.sync()
    torch.cuda.synchronize()
    print("EPOCH %s %s compute_ms %.3f" % (model, arm, (time.perf_counter() - t0) * 1e3 / STEPS))
    for layer in (1, 2):
        l, K = layer - 1, heads[layer - 1]
        zw = dims[layer] * (K if layer == 2 else 1)
        ld = (zw + 31) // 32 * 32
        rb = ld * (2 if bf else 4)
        tag = "%s %s layer%d %dx%d ld %d" % (model, arm, layer, K, zw // K, ld)
        deliver[layer][0]()                                    # (the twins arm: fg_z's twin alone is current again)
        ms, _ = timed2(ctx, "edge", lambda: ctx.apply_edge(layer, da.FORWARD))
        print("RATE %s apply_edge ms %.4f convert_ms 0.0000 gathered_TBps 0.000" % (tag, ms))
        before = ctx.gatmh_row_gather_stats()
        fwd, cv = timed2(ctx, "spmm", lambda: ctx.aggregate(layer, da.FORWARD))
        print("RATE %s forward ms %.4f convert_ms %.4f gathered_TBps %.3f" % (tag, fwd, cv, nin * rb / fwd / 1e9))
        ctx.set_option("gatmh_bwd_phase", 1)
        ctx.aggregate(layer, da.BACKWARD)
        d = [a - b for a, b in zip(ctx.gatmh_row_gather_stats(), before)]
        if d[1] > 0:
            dst, cv = timed2(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD))
            print("RATE %s dst_edge_pass ms %.4f convert_ms %.4f gathered_TBps %.3f" % (tag, dst, cv, nin * rb / dst / 1e9))
        deliver[layer][1]()
        ctx.set_option("gatmh_bwd_phase", 2)
        src, cv = timed2(ctx, "spmm", lambda: ctx.aggregate(layer, da.BACKWARD))
        ctx.set_option("gatmh_bwd_phase", 0)
        print("RATE %s src ms %.4f convert_ms %.4f gathered_TBps %.3f" % (tag, src, cv, nout * rb / src / 1e9))
    if bf:
        st = ctx.gatmh_row_gather_bf16_stats()
        assert st[0] > 0 and st[2] > 0, st
        gs = ctx.halo_bf16_ghosts_stats()
        assert (gs["conversions_skipped"] > 0) == (arm == "twins"), gs
        if arm == "twins":
            s = ctx.gatmh_bf16_ghosts_stats()
            print("STATS %s %s %s" % (model, arm, " ".join("%s %d" % kv for kv in s.items())))
            assert s["widened"] == 0 and s["twin_reads_rows"] > 0 and s["scores_from_twin"] > 0, s
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="the library the parent arm runs on (a build of the parent commit); default: this tree's, new switch off")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--models", nargs="*", default=list(MODELS))
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
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
        got = [ln for ln in r.stdout.splitlines() if ln.split(" ")[0] in ("RATE", "EPOCH", "UNPACK", "STATS", "PART")]
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
        path, parts_path = os.path.join(tmp, "amazon.part"), os.path.join(tmp, "parts.npy")
        part.save(path)
        part.close()
        np.save(parts_path, parts)
        ok = True
        for rnd in range(a.rounds):
            for model in a.models:
                for arm in ARMS:
                    ok = ok and step([model, arm, path, parts_path], a.parent_lib if arm == "parent" else "")
                    if not ok:
                        break
                if not ok:
                    break
            if not ok:
                break
    # medians over the rounds with the spread of the parent's runs, and the twins arm against the parent arm and against fp32
    med = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "RATE":
            med.setdefault((w[1], w[3], w[4], w[6], w[7]), {}).setdefault(w[2], []).append(float(w[9]))     # model, layer, shape, ld, pass
        elif w[0] == "EPOCH":
            med.setdefault((w[1], "-", "-", "-", "compute_epoch"), {}).setdefault(w[2], []).append(float(w[4]))
        elif w[0] == "UNPACK":
            med.setdefault((w[1], w[3], w[4], w[6], "unpack_" + w[7]), {}).setdefault(w[2], []).append(float(w[9]))
    for key, arms in sorted(med.items()):
        if "parent" in arms and "twins" in arms:
            p, t = float(np.median(arms["parent"])), float(np.median(arms["twins"]))
            out = "RATIO %s %s %s ld %s %s parent_ms %.4f (runs %.4f-%.4f) twins_ms %.4f twins_over_parent %.3f%s" % (
                key + (p, min(arms["parent"]), max(arms["parent"]), t, t / p, "" if t < p else "  (NOT FASTER)"))
            if "fp32" in arms:
                f = float(np.median(arms["fp32"]))
                out += " | fp32_ms %.4f (runs %.4f-%.4f) twins_over_fp32 %.3f%s" % (f, min(arms["fp32"]), max(arms["fp32"]), t / f, "" if t < f else "  (NOT FASTER)")
            print(out, flush=True)
            lines.append(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
