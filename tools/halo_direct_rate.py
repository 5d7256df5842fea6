#!/usr/bin/env python3
"""What does option halo_direct_recv take out of an exchange, and does it leave the pack alone?  The synthetic partition of
tools/halo_exact_rate.py (rank 0 of 8, about 1 M send rows in seven sorted per-peer lists, 1 M ghost rows), one context per
option value and width (the option is fixed once the graph is uploaded), the two contexts alternating in one session, ten timed
calls after a warm one per measurement (timing family "halo"), three rounds: the spread between the repeated option-0
measurements is the yardstick's own noise.  Measured per call: the pack (the same kernel and send list under both values), the
unpack of option 0 (what an exchange no longer runs under option 1), and the identity copy dory_halo_unpack still offers under
option 1 to callers with their own transport.  Nothing here measures a link.  Needs no file outside the tree.
GPU box only:  python tools/halo_direct_rate.py [--rows 1048576] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
WIDTHS = (128, 64, 41)
ROUNDS, PEERS = 3, 8


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dorylus_amd as da
    import halo_direct_ref as hd
    from halo_exact_rate import CALLS, synthetic_partition, timed
    n = a.rows
    g = synthetic_partition(n)
    rng = np.random.default_rng(0)
    per = n // (PEERS - 1)
    send = [np.zeros(0, np.uint32)] + [np.sort(rng.integers(0, n, per)).astype(np.uint32) for _ in range(PEERS - 1)]
    # ghost slots dealt to the peers round robin: the wire order is a real permutation of the slots
    slots = [np.zeros(0, np.uint32)] + [np.arange(q, n, PEERS - 1, dtype=np.uint32) for q in range(PEERS - 1)]
    order = np.concatenate(slots)
    send_rows = int(sum(len(x) for x in send))
    lines = [f"# tools/halo_direct_rate.py: {send_rows} send rows, {n} ghost rows, rank 0 of {PEERS}; ms per call (mean of {CALLS} after a warm call),",
             f"# {ROUNDS} rounds alternating the halo_direct_recv 0 and 1 contexts; padded rows (halo_exact_rows 0)",
             "# width ld | pack ms, option 0 (rounds) | pack ms, option 1 (rounds) | unpack ms, option 0 (rounds) = what an exchange drops | "
             "identity unpack ms, option 1 (split entry point only) | pack medians 0 / 1 | spread of the option-0 pack (max - min) | "
             "receive buffer bytes 0 / 1 | verdict on the pack"]
    for w in WIDTHS:
        ctxs, bufs = {}, {}
        for o in (0, 1):
            ctx = da.Context(0)
            ctx.configure(da.GCN, [4, w, 2], 3 * n, 0, PEERS)
            ctx.set_option("halo_direct_recv", o)
            ctx.graph_upload(hd.wired_graph(g, [order, order]) if o else g)
            ctx.preallocate()
            ctx.halo_plan(da.FORWARD, send, slots)
            ctx.fill_uniform(0, "h", 1, -1.0, 1.0)
            ld = ctx.info(0, "h")[2]
            ctxs[o] = ctx
        sbuf = torch.empty(send_rows * ld, device="cuda")
        rbuf = torch.rand(n * ld, device="cuda")
        torch.cuda.synchronize()
        t = {(k, o): [] for k in ("pack", "unpack") for o in (0, 1)}
        for _ in range(ROUNDS):
            for o in (0, 1):
                t[("pack", o)].append(timed(ctxs[o], ctxs[o].halo_pack, 1, da.FORWARD, sbuf.data_ptr()))
                t[("unpack", o)].append(timed(ctxs[o], ctxs[o].halo_unpack, 1, da.FORWARD, rbuf.data_ptr()))
        med = {o: float(np.median(t[("pack", o)])) for o in (0, 1)}
        spread = max(t[("pack", 0)]) - min(t[("pack", 0)])
        verdict = "not slower" if med[1] <= med[0] + spread else "SLOWER beyond the spread"
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        rb = [ctxs[o].get_option("halo_recv_buf_bytes") for o in (0, 1)]
        lines.append(f"{w} {ld} | {fm(t[('pack', 0)])} | {fm(t[('pack', 1)])} | {fm(t[('unpack', 0)])} | {fm(t[('unpack', 1)])} | "
                     f"{med[0]:.4f} / {med[1]:.4f} | {spread:.4f} | {rb[0]} / {rb[1]} | {verdict}")
        print(lines[-1], flush=True)
        del sbuf, rbuf
        for ctx in ctxs.values():
            ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
