#!/usr/bin/env python3
"""Do 16-byte bf16 row gathers pay in the multi-head GAT's row-gather kernels (dory_gatmh_row_gather_bf16_wide)?

The setup of tools/gatmh_bf16_ghosts_rate.py: rank 0 of 8 as a context of an 8-node run with its halo plans, the ghost rows DELIVERED
through dory_halo_unpack (bf16 wire rows of z) and dory_gatmh_bwd_unpack (merged rows of do / st), so that the twins are what the
passes gather; no peer and no link exist, the buffers are filled on the device.  Mode 1, gatmh_bf16_gather = 2, the bf16 wire and the
twins on, gatmh_bwd_phase 1 / 2.
  input `uniform`  the Amazon-size uniform graph (bench.py's synth_incident_edges), no hub splitting
  input `rmat`     the R-MAT graph of tools/gatmh_row_gather_hubs_rate.py, dory_gatmh_row_gather_hub_split(1024)
  arm `parent`     --parent-lib (a build of the parent commit; default: this tree's with the switch off): the narrow bf16 form
  arm `narrow`     this tree's library, the switch off
  arm `wide`       this tree's library, the switch on
Per layer and pass the device time of single dory_aggregate calls (the library's timing family around the pass, the conversion that
belongs to it INCLUDED and also given alone), and a compute epoch driven call by call, wall clock.  The three arms are alternated over
the rounds; every measurement is a child process of its own under a time limit; the first that fails or runs out of time ends the run.
RATIO lines: medians, the runs' ranges, narrow against parent (expected inside the spread: the switch-off path is unchanged) and wide
against narrow (the result); `inside the spread` when the medians differ by no more than the larger of the two arms' ranges.
KERNEL lines: the vector registers of the gatmh_rows8_* kernels, and whether the family's other kernels have the parent's counts.
GPU box only:  python tools/gatmh_row_gather_bf16_wide_rate.py [--out FILE] [--parent-lib LIB] [--rounds 3] [--step-timeout 240]"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
# rows of 128 / 64 and of 64 / 32 floats (the last layer: one head; 32-float rows have no wide form)
MODELS = {"8x16": ([300, 128, 41], [8, 1]), "8x8": ([300, 64, 25], [8, 1])}
GRAPHS = {"uniform": 0, "rmat": 1024}          # input -> chunk_entries of dory_gatmh_row_gather_hub_split
ARMS = ("parent", "narrow", "wide")
WARM, STEPS = 2, 5
LLVM = "/opt/rocm/lib/llvm/bin"


def rate_child(graph, model, arm, path, parts_path):
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
    ctx.gatmh_row_gather_hub_split(GRAPHS[graph])
    part.upload(ctx, parts)
    ctx.preallocate()
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
    labels = np.random.default_rng(2).integers(0, dims[-1], V).astype(np.uint32)
    ctx.labels_upload(labels[g["localToGlobal"]])
    ctx.weights_init_xavier()
    ctx.gatmh_row_gather_bf16(1)
    ctx.set_option("gatmh_bf16_gather", 2)
    ctx.halo_bf16_rows(1)
    ctx.gatmh_halo_bf16(1)
    ctx.halo_bf16_ghosts(1)
    ctx.gatmh_bf16_ghosts(1)
    if arm == "wide":
        ctx.gatmh_row_gather_bf16_wide(1)
    print("PART %s %s %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d" % (graph, model, arm, N, Gs, Gd, nin, nout))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    deliver = {}
    for layer in (1, 2):
        l, K = layer - 1, heads[layer - 1]
        zw = dims[layer] * (K if layer == 2 else 1)
        ld = (zw + 31) // 32 * 32
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
        deliver[layer] = ((lambda layer=layer, z16=z16: ctx.halo_unpack(layer, da.FORWARD, z16.data_ptr())),
                          (lambda l=l, rows=rows: ctx.gatmh_bwd_unpack(l, rows.data_ptr())))
        deliver[layer][0]()
        deliver[layer][1]()

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
    print("EPOCH %s %s %s compute_ms %.3f" % (graph, model, arm, (time.perf_counter() - t0) * 1e3 / STEPS))
    for layer in (1, 2):
        l, K = layer - 1, heads[layer - 1]
        zw = dims[layer] * (K if layer == 2 else 1)
        ld = (zw + 31) // 32 * 32
        rb = ld * 2
        tag = "%s %s %s layer%d %dx%d ld %d" % (graph, model, arm, layer, K, zw // K, ld)
        deliver[layer][0]()                                    # (fg_z's twin alone is current again)
        ctx.apply_edge(layer, da.FORWARD)
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
    st = ctx.gatmh_row_gather_bf16_stats()
    assert st[0] > 0 and st[2] > 0, st
    assert ctx.gatmh_bf16_ghosts_stats()["twin_reads_rows"] > 0
    if GRAPHS[graph]:
        hs = ctx.gatmh_row_gather_hub_split_stats()
        assert hs["fwd"] > 0 and hs["src"] > 0, hs
    if arm != "parent":
        s = ctx.gatmh_row_gather_bf16_wide_stats()
        print("STATS %s %s %s %s" % (graph, model, arm, " ".join("%s %d" % kv for kv in s.items())))
        assert (s["fwd"] > 0 and s["src"] > 0) == (arm == "wide"), s
    ctx.close()


def kernel_notes(lib):
    """{kernel name: (vector registers, spilled)} of the gfx950 code objects inside a library"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        shutil.copy(lib, os.path.join(d, "lib.so"))
        subprocess.run([os.path.join(LLVM, "llvm-objdump"), "--offloading", "lib.so"], cwd=d, check=True, capture_output=True)
        for f in sorted(os.listdir(d)):
            if "gfx950" not in f:
                continue
            notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", f], cwd=d, check=True, capture_output=True, text=True).stdout
            for m in re.finditer(r"\.name:\s+(\S+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)", notes):
                out[m.group(1)] = (int(m.group(2)), int(m.group(3)))
    return out


def kernel_lines(this_lib, parent_lib):
    lines = []
    mine = kernel_notes(this_lib)
    for name, (vgpr, spill) in sorted(mine.items()):
        t = re.search(r"(gatmh_rows8_\w+?_kernel)ILi(\d+)E(?:Lb([01])E)?E", name)
        if t:
            lines.append("KERNEL %s lanes %s%s vgprs %d spilled %d" % (t.group(1), t.group(2), "" if t.group(3) is None else
                                                                       " scores_from_row %s" % t.group(3), vgpr, spill))
    if parent_lib:
        theirs = kernel_notes(parent_lib)
        fam = sorted(k for k in theirs if "gatmh_rows_" in k)
        diff = [k for k in fam if mine.get(k) != theirs[k]]
        lines.append("KERNELS gatmh_rows_* of the parent's library: %d; with the parent's vector register and spill counts in this library: %d%s" %
                     (len(fam), len(fam) - len(diff), "" if not diff else "; DIFFERENT: " + " ".join(diff)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="the library the parent arm runs on (a build of the parent commit); default: this tree's, switch off")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=240)
    ap.add_argument("--models", nargs="*", default=list(MODELS))
    ap.add_argument("--graphs", nargs="*", default=list(GRAPHS))
    ap.add_argument("--child", nargs="+")
    a = ap.parse_args()
    if a.child:
        rate_child(*a.child)
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
            return False
        for ln in r.stdout.splitlines():
            if ln.split(" ")[0] in ("RATE", "EPOCH", "STATS", "PART"):
                say(ln)
        if r.returncode != 0:
            say("# step %s failed (%d): stopping\n%s" % (args[:3], r.returncode, r.stderr[-2000:]))
        flush_out()
        return r.returncode == 0

    for ln in kernel_lines(da.LIB_PATH, a.parent_lib):
        say(ln)
    with tempfile.TemporaryDirectory() as tmp:
        V, E, _ = WORKLOADS["amazon"]
        parts = (np.arange(V, dtype=np.int64) * 8 // V).astype(np.int32)
        parts_path = os.path.join(tmp, "parts.npy")
        np.save(parts_path, parts)
        paths = {}
        for graph in a.graphs:
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
        ok = True
        for rnd in range(a.rounds):
            for graph in a.graphs:
                for model in a.models:
                    for arm in ARMS:
                        ok = ok and step([graph, model, arm, paths[graph], parts_path], a.parent_lib if arm == "parent" else "")
                        if not ok:
                            break
                    if not ok:
                        break
                if not ok:
                    break
            if not ok:
                break
    # medians over the rounds with the runs' ranges: narrow against parent, wide against narrow
    med = {}
    for ln in lines:
        w = ln.split()
        if w[0] == "RATE":
            med.setdefault((w[1], w[2], w[4], w[5], w[7], w[8]), {}).setdefault(w[3], []).append(float(w[10]))   # graph, model, layer, shape, ld, pass
        elif w[0] == "EPOCH":
            med.setdefault((w[1], w[2], "-", "-", "-", "compute_epoch"), {}).setdefault(w[3], []).append(float(w[5]))

    def verdict(x, y):           # arm x against arm y
        mx, my = float(np.median(x)), float(np.median(y))
        spread = max(max(x) - min(x), max(y) - min(y))
        return "x%.3f %s" % (mx / my, "inside the spread" if abs(mx - my) <= spread else "FASTER" if mx < my else "NOT FASTER")
    for key, arms in sorted(med.items()):
        if all(k in arms for k in ARMS):
            say("RATIO %s %s %s %s ld %s %s | " % key + " | ".join("%s_ms %.4f (%.4f..%.4f)" % (k, float(np.median(arms[k])), min(arms[k]), max(arms[k]))
                                                                  for k in ARMS) +
                " | narrow_over_parent %s | wide_over_narrow %s" % (verdict(arms["narrow"], arms["parent"]), verdict(arms["wide"], arms["narrow"])))
    flush_out()


if __name__ == "__main__":
    main()
