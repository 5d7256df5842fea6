#!/usr/bin/env python3
"""What do pack and unpack (K6) cost with dory_halo_bf16_rows against the fp32 kernels, for the same rows?  One context per width on
the synthetic partition of tools/halo_exact_rate.py (rank 0 of 8, seven sorted per-peer send lists with repeats across peers), at the
row counts of profiles/r06_pack_rate.json (an Amazon rank: about 3.15 M send rows and as many ghost rows) and its widths: Amazon 64 and
300 floats, Reddit 128, Friendster 48, 41 -- padded, and exact where that differs.  gcn_bf16_gather = 2 throughout; the switch off and
on alternating, ten timed calls after a warm one per measurement (timing family "halo"), three rounds: the spread between the repeated
switch-off measurements is the yardstick's own noise.  One GPU: kernel times only, nothing here crosses a link.
GPU box only:  python tools/halo_bf16_rate.py [--rows 3145728] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from halo_exact_rate import CALLS, PEERS, ROUNDS, synthetic_partition, timed  # noqa: E402

CASES = ((64, 0), (300, 0), (300, 1), (128, 0), (48, 0), (48, 1), (41, 0), (41, 1))      # (width, halo_exact_rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=3 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dorylus_amd as da
    n = a.rows
    g = synthetic_partition(n)
    rng = np.random.default_rng(0)
    per = n // (PEERS - 1)
    send = [np.zeros(0, np.uint32)] + [np.sort(rng.integers(0, n, per)).astype(np.uint32) for _ in range(PEERS - 1)]
    slots = [np.zeros(0, np.uint32)] + [x.astype(np.uint32) for x in np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)]
    send_rows = int(sum(len(x) for x in send))
    lines = [f"# tools/halo_bf16_rate.py: {send_rows} send rows, {n} ghost rows, rank 0 of {PEERS}; ms per call (mean of {CALLS} after a warm call),",
             f"# {ROUNDS} rounds alternating dory_halo_bf16_rows 0 / 1 under gcn_bf16_gather = 2; MB = bytes of the packed side per call",
             "# width exact | row bytes fp32 / bf16 | pack MB fp32 / bf16 | pack ms fp32 (rounds) | pack ms bf16 (rounds) | unpack ms fp32 (rounds) | "
             "unpack ms bf16 (rounds) | pack ms medians fp32 / bf16, ratio | unpack ms medians fp32 / bf16, ratio | spread of fp32 pack, unpack | verdict"]
    ctx, cur = None, None
    for w, exact in CASES:
        if cur != w:
            if ctx:
                ctx.close()
            ctx = da.Context(0)
            ctx.configure(da.GCN, [4, w, 2], 3 * n, 0, PEERS)
            ctx.set_option("gcn_bf16_gather", 2)
            ctx.graph_upload(g)
            ctx.preallocate()
            ctx.halo_plan(da.FORWARD, send, slots)
            ctx.fill_uniform(0, "h", 1, -1.0, 1.0)
            cur = w
        ctx.set_option("halo_exact_rows", exact)
        ld = ctx.info(0, "h")[2]
        sbuf = torch.empty(send_rows * ld, device="cuda")
        rbuf = torch.rand(n * ld, device="cuda")           # (as bf16 pairs: finite or not, the unpack only widens)
        torch.cuda.synchronize()
        t = {(k, o): [] for k in ("pack", "unpack") for o in (0, 1)}
        rowb = {}
        for _ in range(ROUNDS):
            for o in (0, 1):
                ctx.halo_bf16_rows(o)
                eb, re = ctx.halo_wire_row(1, da.FORWARD)
                rowb[o] = eb * re
                t[("pack", o)].append(timed(ctx, ctx.halo_pack, 1, da.FORWARD, sbuf.data_ptr()))
                t[("unpack", o)].append(timed(ctx, ctx.halo_unpack, 1, da.FORWARD, rbuf.data_ptr()))
        med = {k: float(np.median(v)) for k, v in t.items()}
        spread = {k: max(t[(k, 0)]) - min(t[(k, 0)]) for k in ("pack", "unpack")}
        slower = [k for k in ("pack", "unpack") if med[(k, 1)] > med[(k, 0)] + 2 * spread[k]]
        verdict = "bf16 not slower" if not slower else "bf16 SLOWER beyond twice the spread: " + ", ".join(slower)
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        lines.append(f"{w} {exact} | {rowb[0]} / {rowb[1]} | {send_rows * rowb[0] / 1e6:.1f} / {send_rows * rowb[1] / 1e6:.1f} | "
                     f"{fm(t[('pack', 0)])} | {fm(t[('pack', 1)])} | {fm(t[('unpack', 0)])} | {fm(t[('unpack', 1)])} | "
                     f"{med[('pack', 0)]:.4f} / {med[('pack', 1)]:.4f}, {med[('pack', 1)] / med[('pack', 0)]:.3f} | "
                     f"{med[('unpack', 0)]:.4f} / {med[('unpack', 1)]:.4f}, {med[('unpack', 1)] / med[('unpack', 0)]:.3f} | "
                     f"{spread['pack']:.4f}, {spread['unpack']:.4f} | {verdict}")
        print(lines[-1], flush=True)
        del sbuf, rbuf
    if ctx:
        ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
