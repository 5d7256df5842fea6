#!/usr/bin/env python3
"""What does the fused halo pack's bf16 form (dory_halo_fused_pack_bf16) cost the producing GEMM, against the pair it replaces --
the GEMM plus the bf16 pack kernel (gather_rows_bf16_kernel)?  One context per shape on a synthetic partition (rank 0 of 8, every
local row listed for 1 peer, then for 3 peers), gather mode 2, dory_halo_bf16_rows and dory_halo_fused_pack on; device time by
events (the library's timing families): per shape
  (a) the producer with the new switch off   (family "gemm" of one dory_apply_vertex: the product that travels and, for the NT
                                              shape, the two other GEMMs of that call -- the same ones in (a) and (c))
  (b) the bf16 pack kernel alone             (family "halo" of dory_halo_pack into a device buffer: it follows the rule)
  (c) the producer with the new switch on    (the bf16 send GEMM alone)
ten timed calls after a warm one per measurement, ROUNDS rounds alternating (a) (b) (c): the baseline is (a) + (b), the candidate (c),
the spread of the repeated (a) + (b) is the yardstick's own noise.  The rows the last producer left are then sent once and must be
counted as a fused bf16 exchange of the right size.
Every step -- one shape at one fan-out -- runs in a child process of its own under a time limit; the first step that fails or
runs out of time ends the run.  With a library from before the feature (DORY_LIB_PATH) only (a) and (b) are measured.  Needs no
file outside the tree.  No link and no second GPU is involved: nothing here says anything about an exchange's transfer.
GPU box only:  python tools/halo_fused_bf16_rate.py [--rows 1048576] [--out FILE] [--step-timeout 150]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, CALLS, PEERS = 3, 10, 8
# name, model, dims, source tensor, input tensor, producer call (layer, dir), direction of the exchange, halo_exact_rows
SHAPES = (
    ("NN+tanh 602->128", "GCN", [602, 128, 2], (0, "h"), (0, "ah"), (0, 0), 0, 0),
    ("NT 41->128", "GCN", [4, 128, 41], (1, "grad"), (1, "ah"), (1, 0), 1, 0),
    ("NN 300->64", "GAT", [300, 64, 2], (0, "z"), (0, "h"), (0, 0), 0, 0),
    ("NN 128->48 padded", "GAT", [128, 48, 2], (0, "z"), (0, "h"), (0, 0), 0, 0),
    ("NN 128->48 exact", "GAT", [128, 48, 2], (0, "z"), (0, "h"), (0, 0), 0, 1),
    ("NN 128->41 padded", "GAT", [128, 41, 2], (0, "z"), (0, "h"), (0, 0), 0, 0),
    ("NN 128->41 exact", "GAT", [128, 41, 2], (0, "z"), (0, "h"), (0, 0), 0, 1),
    ("NN 128->300 padded", "GAT", [128, 300, 2], (0, "z"), (0, "h"), (0, 0), 0, 0),
    ("NN 128->300 exact", "GAT", [128, 300, 2], (0, "z"), (0, "h"), (0, 0), 0, 1),
)
HEADER = ("# shape | peers per row | send rows | packed MB (bf16) | (a) producer, switch off (rounds) | (b) bf16 pack kernel (rounds) | "
          "(c) producer, switch on (rounds) | medians a + b / c | c - (a + b) | spread of a + b | verdict")


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


def one_step(n, si, per_row):
    """one shape at one fan-out, in this process: prints its line"""
    import torch
    import dorylus_amd as da
    from halo_exact_rate import synthetic_partition
    name, model, dims, src, inp, prod, xdir, exact = SHAPES[si]
    g = synthetic_partition(n)
    have = hasattr(da.load(), "dory_halo_fused_pack_bf16")
    slots = [np.zeros(0, np.uint32)] + [x.astype(np.uint32) for x in np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)]
    own = np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)      # every row once (to the peer that owns its block), or to three peers
    send = [np.zeros(0, np.uint32)] + [np.sort(np.concatenate([own[(q + k) % (PEERS - 1)] for k in range(per_row)])) for q in range(PEERS - 1)]
    send_rows = int(sum(len(x) for x in send))
    ctx = da.Context(0)
    ctx.configure(getattr(da, model), dims, 3 * n, 0, PEERS)
    ctx.set_option("halo_exact_rows", exact)
    ctx.graph_upload(g)
    ctx.preallocate()
    ctx.halo_plan(xdir, send, slots)
    ctx.weights_init_xavier()
    ctx.fill_uniform(inp[0], inp[1], 1, -1.0, 1.0)
    if model == "GCN":
        ctx.set_option("gcn_bf16_gather", 2)
    else:
        ctx.gat_bf16_gather(2)
    ctx.halo_bf16_rows(1)
    ctx.halo_fused_pack(1)
    sent = []
    ctx.set_host_transport(lambda s_, sc, so, r_, rc, ro: sent.append(int(sc.sum())), lambda buf: None)
    eb, re = ctx.halo_wire_row(1, xdir)
    assert eb == 2, "the exchange does not ship bf16"
    sbuf = torch.empty(send_rows * re // 2 + 16, device="cuda")
    torch.cuda.synchronize()
    t = {"a": [], "b": [], "c": []}
    for _ in range(ROUNDS):
        if have:
            ctx.halo_fused_pack_bf16(0)
        t["a"].append(timed(ctx, "gemm", ctx.apply_vertex, *prod))
        t["b"].append(timed(ctx, "halo", ctx.halo_pack, 1, xdir, sbuf.data_ptr()))
        if have:
            ctx.halo_fused_pack_bf16(1)
            t["c"].append(timed(ctx, "gemm", ctx.apply_vertex, *prod))
    if have:       # the rows the last producer left are the ones that travel: one exchange, counted as fused and as bf16
        ctx.halo_exchange(1, xdir)
        ctx.sync()
        assert ctx.halo_fused_pack_bf16_stats() == (1, send_rows) and sent == [send_rows * re // 2], (ctx.halo_fused_pack_bf16_stats(), sent)
    fm = lambda xs: " ".join(f"{x:.4f}" for x in xs) if xs else "-"
    pair = [a + b for a, b in zip(t["a"], t["b"])]
    mp, spread = float(np.median(pair)), max(pair) - min(pair)
    if have:
        mc = float(np.median(t["c"]))
        verdict = ("cheaper than the pair" if mc <= mp - spread else "inside the pair's spread" if mc <= mp + spread
                   else "SLOWER than the GEMM plus the pack it replaces")
        tail = f"{mp:.4f} / {mc:.4f} | {mc - mp:+.4f} | {spread:.4f} | {verdict}"
    else:
        tail = f"{mp:.4f} / - | - | {spread:.4f} | -"
    print(f"{name} | {per_row} | {send_rows} | {send_rows * re * 2 / 1e6:.1f} | {fm(t['a'])} | {fm(t['b'])} | {fm(t['c'])} | {tail}", flush=True)
    del sbuf
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds one shape at one fan-out may take")
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)      # (the child: shape index, peers per row)
    a = ap.parse_args()
    if a.step:
        one_step(a.rows, *a.step)
        return 0
    lines = [f"# tools/halo_fused_bf16_rate.py: {a.rows} local rows, rank 0 of {PEERS}, library {os.environ.get('DORY_LIB_PATH', 'of the tree')};",
             f"# ms per call (mean of {CALLS} after a warm call), {ROUNDS} rounds alternating a / b / c; no link, one GPU", HEADER]
    print("\n".join(lines), flush=True)
    rc = 0
    for si in range(len(SHAPES)):
        for per_row in (1, 3):
            try:       # a fresh child process per step, under its own time limit; the first failure ends the run
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--step", str(si), str(per_row)],
                                   capture_output=True, text=True, timeout=a.step_timeout)
            except subprocess.TimeoutExpired:
                lines.append(f"# STOPPED: {SHAPES[si][0]} | {per_row} ran longer than {a.step_timeout} s")
                rc = 124
                break
            if r.returncode != 0:
                lines.append(f"# STOPPED: {SHAPES[si][0]} | {per_row} ended with status {r.returncode}\n# " + r.stderr.strip()[-1500:].replace("\n", "\n# "))
                rc = r.returncode
                break
            lines.append(r.stdout.strip().splitlines()[-1])
            print(lines[-1], flush=True)
        if rc:
            print(lines[-1], flush=True)
            break
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
