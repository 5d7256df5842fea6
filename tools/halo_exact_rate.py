#!/usr/bin/env python3
"""What do pack and unpack (K6) cost with option halo_exact_rows against the padded form, for the same rows?  One context per
width on a synthetic partition (rank 0 of 8, about 1 M send rows in seven sorted per-peer lists with repeats across peers, 1 M
ghost rows), options 0 and 1 alternating, ten timed calls after a warm one per measurement (timing family "halo"), three
rounds: the spread between the repeated option-0 measurements is the yardstick's own noise.  Needs no file outside the tree.
GPU box only:  python tools/halo_exact_rate.py [--rows 1048576] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
WIDTHS = (41, 25, 48, 602)
ROUNDS, CALLS, PEERS = 3, 10, 8


def synthetic_partition(n):
    """n local vertices on a ring, n ghost sources and n ghost destinations with one edge each: the dict Context.graph_upload takes"""
    v = np.arange(n, dtype=np.uint32)
    ptr = (2 * np.arange(n + 1)).astype(np.uint64)
    in_idx = np.stack([(v + 1) % n, n + v], 1).reshape(-1).astype(np.uint32)       # a local and a ghost source per destination
    out_idx = np.stack([(v + n - 1) % n, n + v], 1).reshape(-1).astype(np.uint32)  # a local and a ghost destination per source
    val = np.full(2 * n, 0.5, np.float32)
    return dict(localVtxCnt=n, globalVtxCnt=3 * n, srcGhostCnt=n, dstGhostCnt=n, colPtr=ptr, rowIdx=in_idx, cscVal=val,
                rowPtr=ptr, colIdx=out_idx, csrVal=val, norm=np.full(n, 0.5, np.float32))


def timed(ctx, fn, *args):
    fn(*args)
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(CALLS):
        fn(*args)
    ctx.sync()
    ms, n = ctx.timing_get("halo")
    ctx.timing_enable(False)
    assert n == CALLS, n
    return ms / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
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
    lines = [f"# tools/halo_exact_rate.py: {send_rows} send rows, {n} ghost rows, rank 0 of {PEERS}; ms per call (mean of {CALLS} after a warm call),",
             f"# {ROUNDS} rounds alternating halo_exact_rows 0 / 1; bytes per call = rows x width x 4 on the packed side",
             "# width ld | pack MB 0 / 1 | unpack MB 0 / 1 | pack ms 0 (rounds) | pack ms 1 (rounds) | unpack ms 0 (rounds) | unpack ms 1 (rounds) |"
             " pack+unpack ms 0 / 1 (medians) | ratio 1/0 | spread of option 0 (max - min of pack+unpack over the rounds) | verdict"]
    for w in WIDTHS:
        ctx = da.Context(0)
        ctx.configure(da.GCN, [4, w, 2], 3 * n, 0, PEERS)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.halo_plan(da.FORWARD, send, slots)
        ctx.fill_uniform(0, "h", 1, -1.0, 1.0)
        ld = ctx.info(0, "h")[2]
        sbuf = torch.empty(send_rows * ld, device="cuda")
        rbuf = torch.rand(n * ld, device="cuda")
        torch.cuda.synchronize()
        t = {(k, o): [] for k in ("pack", "unpack") for o in (0, 1)}
        for _ in range(ROUNDS):
            for o in (0, 1):
                ctx.set_option("halo_exact_rows", o)
                t[("pack", o)].append(timed(ctx, ctx.halo_pack, 1, da.FORWARD, sbuf.data_ptr()))
                t[("unpack", o)].append(timed(ctx, ctx.halo_unpack, 1, da.FORWARD, rbuf.data_ptr()))
        both = {o: [p + u for p, u in zip(t[("pack", o)], t[("unpack", o)])] for o in (0, 1)}
        med = {o: float(np.median(both[o])) for o in (0, 1)}
        spread = max(both[0]) - min(both[0])
        verdict = "not slower" if med[1] <= med[0] + 2 * spread else "SLOWER beyond twice the spread"
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        lines.append(f"{w} {ld} | {send_rows * ld * 4 / 1e6:.1f} / {send_rows * w * 4 / 1e6:.1f} | {n * ld * 4 / 1e6:.1f} / {n * w * 4 / 1e6:.1f} | "
                     f"{fm(t[('pack', 0)])} | {fm(t[('pack', 1)])} | {fm(t[('unpack', 0)])} | {fm(t[('unpack', 1)])} | "
                     f"{med[0]:.4f} / {med[1]:.4f} | {med[1] / med[0]:.3f} | {spread:.4f} | {verdict}")
        print(lines[-1], flush=True)
        del sbuf, rbuf
        ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
