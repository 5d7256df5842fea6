#!/usr/bin/env python3
"""Do 16-byte bf16 row gathers pay in K1, the row gather a partitioned rank of a large graph runs (dory_k1_bf16_wide)?

The setup of tools/gatmh_row_gather_bf16_wide_rate.py: rank 0 of 8 as a GCN context of an 8-node run with its halo plans,
spmm_variant = 0 (K1), the ghost rows DELIVERED through dory_halo_unpack in both directions (bf16 wire rows, so that the twins are what
the bf16 arms gather; fp32 rows for the fp32 arm); no peer and no link exist, the buffers are filled on the device.
  input `uniform`   the Amazon-size uniform graph (bench.py's synth_incident_edges), rows of 300 (ld 320), 128 and 64 floats
  input `rmat`      the R-MAT graph of tools/gatmh_row_gather_hubs_rate.py (hub rows: K1's long-row kernels run), rows of 128 floats
  arm `fp32`        this tree's library, gcn_bf16_gather = 0
  arm `parent`      --parent-lib (a build of the parent commit; default: this tree's with the switch off), gcn_bf16_gather = 2: narrow
  arm `narrow`      this tree's library, gcn_bf16_gather = 2, the switch off
  arm `wide`        this tree's library, gcn_bf16_gather = 2, the switch on
  arm `wide16x3`    --alt-lib (a build of this tree with EXTRA=-DDORY_K1_WIDE_CH48_16X3=1: rows of 33..48 chunks on (16, 3) instead of
                    (64, 1)), the switch on; ld 320 only, and only where the library is given
Per width the device time of single dory_aggregate calls, layer 1 forward (h@0, fg@1) and backward (grad@1, bg@0): the library's
timing family around K1's launches PLUS the conversion of the N local rows into the shadow rows (also given alone).  The arms are
alternated over the rounds; every measurement is a child process of its own under a time limit; the first that fails or runs out of
time ends the run.  RATIO lines: medians, the runs' ranges, narrow against parent (expected inside the spread: the switch-off path is
unchanged), narrow against fp32 and wide against narrow (the results); `inside the spread` when the medians differ by no more than the
larger of the two arms' ranges.  KERNEL lines: the vector registers of the spmm_rows_bf16x8_kernel instantiations, and whether K1's
other kernels have the parent's counts.
GPU box only:  python tools/k1_bf16_wide_rate.py [--out FILE] [--parent-lib LIB] [--alt-lib LIB] [--rounds 3] [--step-timeout 120]"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
WIDTHS = {"uniform": (300, 128, 64), "rmat": (128,)}
ARMS = ("fp32", "parent", "narrow", "wide", "wide16x3")
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
    bf = arm != "fp32"
    ctx = da.Context(0)
    ctx.configure(da.GCN, [16, W, 8], V, 0, 8)
    ctx.set_option("spmm_variant", 0)
    ctx.set_option("gcn_bf16_gather", 2 if bf else 0)
    part.upload(ctx, parts)
    ctx.preallocate()
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0, g["localToGlobal"])
    ctx.fill_uniform(1, "grad", 2, -1.0, 1.0, g["localToGlobal"])
    ctx.halo_bf16_rows(1)
    ctx.halo_bf16_ghosts(1)
    if arm.startswith("wide"):
        ctx.k1_bf16_wide(1)
    ld = (W + 31) // 32 * 32
    print("PART %s %d %s local %d src_ghosts %d dst_ghosts %d in_edges %d out_edges %d" % (graph, W, arm, N, Gs, Gd, nin, nout))
    gen = torch.Generator(device="cuda")
    gen.manual_seed(3)
    keep = []
    for direction, G in ((da.FORWARD, Gs), (da.BACKWARD, Gd)):
        eb, n = ctx.halo_wire_row(1, direction)
        assert (eb, n) == ((2, ld) if bf else (4, ld)), (eb, n, ld)
        rows = torch.rand((G, n), device="cuda", generator=gen) * 2 - 1
        rows[:, W:] = 0
        rows = rows.to(torch.bfloat16) if bf else rows
        torch.cuda.synchronize()
        ctx.halo_unpack(1, direction, rows.data_ptr())
        keep.append(rows)
    ctx.sync()
    twin0 = ctx.halo_bf16_ghosts_stats()["conversions_skipped"]
    for direction, name, edges in ((da.FORWARD, "forward", nin), (da.BACKWARD, "backward", nout)):
        fn = lambda: ctx.aggregate(1, direction)
        fn()
        ctx.sync()
        ctx.timing_reset()
        ctx.timing_enable(True)
        for _ in range(CALLS):
            fn()
        ctx.sync()
        ms, n = ctx.timing_get("spmm")
        cv, _ = ctx.timing_get("bf16_convert")
        ctx.timing_enable(False)
        assert n
        ms, cv = ms / CALLS, cv / CALLS
        rb = ld * (2 if bf else 4)
        print("RATE %s %d %s ld %d %s ms %.4f k1_ms %.4f convert_ms %.4f gathered_TBps %.3f" %
              (graph, W, arm, ld, name, ms + cv, ms, cv, edges * rb / ms / 1e9))
    assert ctx.get_option("spmm_launches_k1") == 2 * (CALLS + 1) and ctx.get_option("spmm_launches_k1s") == 0
    if bf:       # every bf16 aggregation gathered its ghost rows from the twin
        assert ctx.halo_bf16_ghosts_stats()["conversions_skipped"] - twin0 == 2 * (CALLS + 1)
    if arm != "parent":
        s = ctx.k1_bf16_wide_stats()
        print("STATS %s %d %s %s" % (graph, W, arm, " ".join("%s %d" % kv for kv in s.items())))
        assert s == {"wide": 2 * (CALLS + 1) if arm.startswith("wide") else 0, "narrow_while_on": 0}, s
    ctx.close()


def kernel_lines(this_lib, parent_lib, alt_lib):
    from gatmh_row_gather_bf16_wide_rate import kernel_notes
    lines = []
    mine = kernel_notes(this_lib)
    for tag, notes in (("", mine), ("alt-lib ", kernel_notes(alt_lib) if alt_lib else {})):
        for name, (vgpr, spill) in sorted(notes.items()):
            t = re.search(r"spmm_rows_bf16x8_kernelILi(\d+)ELi(\d+)EE", name)
            if t:
                lines.append("KERNEL %sspmm_rows_bf16x8_kernel lanes %s chunks %s vgprs %d spilled %d" % (tag, t.group(1), t.group(2), vgpr, spill))
    if parent_lib:
        theirs = kernel_notes(parent_lib)
        fam = sorted(k for k in theirs if "spmm_rows" in k or "spmm_longrow" in k)
        diff = [k for k in fam if mine.get(k) != theirs[k]]
        lines.append("KERNELS spmm_rows* / spmm_longrow* of the parent's library: %d; with the parent's vector register and spill counts in this library: %d%s" %
                     (len(fam), len(fam) - len(diff), "" if not diff else "; DIFFERENT: " + " ".join(diff)))
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--parent-lib", default="", help="the library the parent arm runs on (a build of the parent commit); default: this tree's, switch off")
    ap.add_argument("--alt-lib", default="", help="a build of this tree with -DDORY_K1_WIDE_CH48_16X3=1: the arm wide16x3 at ld 320")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--step-timeout", type=int, default=120)
    ap.add_argument("--graphs", nargs="*", default=list(WIDTHS))
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
            flush_out()
            return False
        for ln in r.stdout.splitlines():
            if ln.split(" ")[0] in ("RATE", "STATS", "PART"):
                say(ln)
        if r.returncode != 0:
            say("# step %s failed (%d): stopping\n%s" % (args[:3], r.returncode, r.stderr[-2000:]))
        flush_out()
        return r.returncode == 0

    for ln in kernel_lines(da.LIB_PATH, a.parent_lib, a.alt_lib):
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
                for W in WIDTHS[graph]:
                    for arm in ARMS:
                        if arm == "wide16x3" and not (a.alt_lib and W == 300):
                            continue
                        lib = a.parent_lib if arm == "parent" else a.alt_lib if arm == "wide16x3" else ""
                        ok = ok and step([graph, str(W), arm, paths[graph], parts_path], lib)
                        if not ok:
                            break
                    if not ok:
                        break
                if not ok:
                    break
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
        if all(k in arms for k in ARMS[:4]):
            ln = "RATIO %s %s ld %s %s | " % key + " | ".join("%s_ms %.4f (%.4f..%.4f)" % (k, float(np.median(arms[k])), min(arms[k]), max(arms[k]))
                                                              for k in ARMS if k in arms)
            ln += " | narrow_over_parent %s | narrow_over_fp32 %s | wide_over_narrow %s" % (
                verdict(arms["narrow"], arms["parent"]), verdict(arms["narrow"], arms["fp32"]), verdict(arms["wide"], arms["narrow"]))
            if "wide16x3" in arms:
                ln += " | wide16x3_over_wide %s" % verdict(arms["wide16x3"], arms["wide"])
            say(ln)
    flush_out()


if __name__ == "__main__":
    main()
