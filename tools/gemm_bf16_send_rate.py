#!/usr/bin/env python3
"""What do the send forms of K2b and K2c (dory_gemm_bf16_send; csrc/gemm_bf16.hip, gemm_bf16_split.hip, gemm_bf16_tile.hpp) buy a product
that feeds a halo exchange?  One context per step on a synthetic partition (rank 0 of 8, every local row listed for 1 peer, then for 3
peers -- the send plan of tools/halo_fused_bf16_rate.py), dory_gemm_bf16 mode 1; device time by events (the library's timing families)
of the producing dory_apply_vertex (family "gemm": the product that travels and, for the NT shape, the other GEMMs of that call -- the
same ones in every arm) plus, where one runs, the pack kernel (family "halo" of dory_halo_pack into a device buffer):
  A    dory_halo_fused_pack on, the new switch 0: K2's fp32 send kernel -- launch for launch what the parent's library runs
  B    dory_halo_fused_pack off: K2b's plain kernel + the pack kernel          C    fused pack on, the switch on: K2b's send kernel
  B'   as B under dory_gemm_bf16_split: K2c's plain kernel + the pack kernel   C'   K2c's send kernel
ten timed calls after a warm one per measurement, ROUNDS rounds alternating A B C B' C'; a ratio is `inside the spread` when the medians
differ by no more than the larger range of the two series.  The counters must say which kernels ran.  Shapes: the sent products of
Reddit (602 -> 128 NN + tanh, 41 -> 128 NT), an Amazon rank (300 -> 64, 64 -> 64) and Friendster (256 -> 48), each on the padded fp32 wire
and the bf16 wire (gather mode 2, dory_halo_bf16_rows, dory_halo_fused_pack_bf16).
Every step -- one shape, wire and fan-out -- runs in a child process of its own under a time limit; the first step that fails or runs out
of time ends the run, and the lines it did not reach are named.  No link and no second GPU is involved.
GPU box only:  python tools/gemm_bf16_send_rate.py [--rows 1048576] [--fanouts 1 3] [--out FILE] [--step-timeout 150]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, CALLS, PEERS = 3, 10, 8
# name, model, dims, input tensor, producer call (layer, dir), direction of the exchange
SHAPES = (
    ("reddit NN+tanh 602->128", "GCN", [602, 128, 2], (0, "ah"), (0, 0), 0),
    ("reddit NT 41->128", "GCN", [4, 128, 41], (1, "ah"), (1, 0), 1),
    ("amazon/8 NN 300->64", "GAT", [300, 64, 2], (0, "h"), (0, 0), 0),
    ("amazon/8 NN 64->64", "GAT", [64, 64, 2], (0, "h"), (0, 0), 0),
    ("friendster/32 NN 256->48", "GAT", [256, 48, 2], (0, "h"), (0, 0), 0),
)
WIRES = ("fp32", "bf16")
HEADER = ("# shape | wire | peers per row | send rows | A K2 send (rounds) | B K2b + pack (rounds) | C K2b send (rounds) | B' K2c + pack (rounds) | "
          "C' K2c send (rounds) | medians A B C B' C' | C/A | C/B | C'/A | C'/B'")


def timed(ctx, family, fn, *args):
    fn(*args)
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(CALLS):
        fn(*args)
    ctx.sync()
    ms, n = ctx.timing_get(family)
    ctx.timing_enable(False)
    assert n and n % CALLS == 0, (family, n)
    return ms / CALLS


def verdict(x, y):
    mx, my = float(np.median(x)), float(np.median(y))
    spread = max(max(x) - min(x), max(y) - min(y))
    return "x%.3f %s" % (mx / my, "inside the spread" if abs(mx - my) <= spread else "FASTER" if mx < my else "NOT FASTER")


def one_step(n, si, wire, per_row):
    """one shape on one wire at one fan-out, in this process: prints its line"""
    import torch
    import dorylus_amd as da
    from halo_exact_rate import synthetic_partition
    name, model, dims, inp, prod, xdir = SHAPES[si]
    g = synthetic_partition(n)
    slots = [np.zeros(0, np.uint32)] + [x.astype(np.uint32) for x in np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)]
    own = np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)      # every row once (to the peer that owns its block), or to three peers
    send = [np.zeros(0, np.uint32)] + [np.sort(np.concatenate([own[(q + k) % (PEERS - 1)] for k in range(per_row)])) for q in range(PEERS - 1)]
    send_rows = int(sum(len(x) for x in send))
    ctx = da.Context(0)
    ctx.configure(getattr(da, model), dims, 3 * n, 0, PEERS)
    ctx.graph_upload(g)
    ctx.preallocate()
    ctx.halo_plan(xdir, send, slots)
    ctx.weights_init_xavier()
    ctx.fill_uniform(inp[0], inp[1], 1, -1.0, 1.0)
    if wire == "bf16":
        if model == "GCN":
            ctx.set_option("gcn_bf16_gather", 2)
        else:
            ctx.gat_bf16_gather(2)
        ctx.halo_bf16_rows(1)
        ctx.halo_fused_pack_bf16(1)
    ctx.gemm_bf16(1)
    ctx.set_host_transport(lambda s_, sc, so, r_, rc, ro: None, lambda buf: None)
    eb, re = ctx.halo_wire_row(1, xdir)
    assert eb == (2 if wire == "bf16" else 4), "the exchange does not ship the wire asked for"
    sbuf = torch.empty(send_rows * re * eb // 4 + 16, device="cuda")
    torch.cuda.synchronize()

    def arm(fused, send_on, split):
        ctx.halo_fused_pack(fused)
        ctx.gemm_bf16_send(send_on)
        ctx.gemm_bf16_split(split)
        before = (ctx.gemm_bf16_send_stats()["send_launches"], ctx.gemm_bf16_stats()["fp32_while_on"], ctx.gemm_bf16_split_stats()["split_launches"])
        ms = timed(ctx, "gemm", ctx.apply_vertex, *prod)
        after = (ctx.gemm_bf16_send_stats()["send_launches"], ctx.gemm_bf16_stats()["fp32_while_on"], ctx.gemm_bf16_split_stats()["split_launches"])
        d = [y - x for x, y in zip(before, after)]
        assert d[0] == (CALLS + 1) * send_on and d[1] == (CALLS + 1) * (fused and not send_on) and (d[2] > 0) == bool(split), (fused, send_on, split, d)
        if not fused:
            ms += timed(ctx, "halo", ctx.halo_pack, 1, xdir, sbuf.data_ptr())
        return ms
    t = {k: [] for k in ("A", "B", "C", "B'", "C'")}
    for _ in range(ROUNDS):
        t["A"].append(arm(1, 0, 0))
        t["B"].append(arm(0, 0, 0))
        t["C"].append(arm(1, 1, 0))
        t["B'"].append(arm(0, 0, 1))
        t["C'"].append(arm(1, 1, 1))
    ctx.halo_exchange(1, xdir)      # the rows the last producer left travel: one fused exchange of the right size
    ctx.sync()
    assert ctx.halo_fused_pack_stats()[:2] == (1, send_rows), ctx.halo_fused_pack_stats()
    fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
    med = " ".join(f"{float(np.median(t[k])):.4f}" for k in t)
    A, B, C_, B2, C2 = (t[k] for k in ("A", "B", "C", "B'", "C'"))
    print(f"{name} | {wire} | {per_row} | {send_rows} | {fm(A)} | {fm(B)} | {fm(C_)} | {fm(B2)} | {fm(C2)} | {med} | "
          f"{verdict(C_, A)} | {verdict(C_, B)} | {verdict(C2, A)} | {verdict(C2, B2)}", flush=True)
    del sbuf
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--fanouts", type=int, nargs="+", default=[1, 3], help="peers per row")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds one step may take")
    ap.add_argument("--step", nargs=3, default=None, help=argparse.SUPPRESS)      # (the child: shape index, wire, peers per row)
    a = ap.parse_args()
    if a.step:
        one_step(a.rows, int(a.step[0]), a.step[1], int(a.step[2]))
        return 0
    lines = [f"# tools/gemm_bf16_send_rate.py: {a.rows} local rows, rank 0 of {PEERS}, dory_gemm_bf16 mode 1;",
             f"# ms per call (mean of {CALLS} after a warm call), {ROUNDS} rounds alternating A B C B' C'; no link, one GPU", HEADER]

    def flush():
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    print("\n".join(lines), flush=True)
    steps = [(si, wire, per_row) for si in range(len(SHAPES)) for wire in WIRES for per_row in a.fanouts]
    rc = 0
    for i, (si, wire, per_row) in enumerate(steps):
        what = f"{SHAPES[si][0]} | {wire} | {per_row}"
        try:       # a fresh child process per step, under its own time limit; the first failure ends the run
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--step", str(si), wire, str(per_row)],
                               capture_output=True, text=True, timeout=a.step_timeout)
            if r.returncode != 0:
                lines.append(f"# STOPPED: {what} ended with status {r.returncode}\n# " + r.stderr.strip()[-1500:].replace("\n", "\n# "))
                rc = r.returncode
            else:
                lines.append(r.stdout.strip().splitlines()[-1])
        except subprocess.TimeoutExpired:
            lines.append(f"# STOPPED: {what} ran longer than {a.step_timeout} s")
            rc = 124
        print(lines[-1], flush=True)
        if rc:
            not_run = [f"# NOT RUN: {SHAPES[s][0]} | {w} | {p}" for s, w, p in steps[i + 1:]]
            lines += not_run
            print("\n".join(not_run), flush=True)
            break
        flush()
    flush()
    return rc


if __name__ == "__main__":
    sys.exit(main())
