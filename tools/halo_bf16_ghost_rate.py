#!/usr/bin/env python3
"""What does the unpack cost when the received bf16 rows stay bf16 (dory_halo_bf16_ghosts: scatter_rows_bf16_keep_kernel into the twin)
against the widening unpack of dory_halo_bf16_rows alone (scatter_rows_bf16_kernel into the fp32 ghost tensor), for the same rows?
The shapes of tools/halo_bf16_rate.py: 3.15 M ghost rows; 64, 300, 128, 48 and 41 floats, padded and exact where that differs.
gcn_bf16_gather = 2 and dory_halo_bf16_rows = 1 throughout, the new switch off and on alternating, ten timed dory_halo_unpack calls
after a warm one per measurement (timing family "halo"), three rounds: the spread of the repeated switch-off measurements is the
yardstick's own noise.  Also timed, once per shape: the dense widening a reader of fp32 rows pays (timing key "bf16_widen").  One
GPU: kernel times only, nothing here crosses a link.
GPU box only:  python tools/halo_bf16_ghost_rate.py [--rows 3145728] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from halo_bf16_rate import CASES  # noqa: E402
from halo_exact_rate import CALLS, PEERS, ROUNDS, synthetic_partition, timed  # noqa: E402


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
    lines = [f"# tools/halo_bf16_ghost_rate.py: {n} ghost rows, rank 0 of {PEERS}; ms per dory_halo_unpack (mean of {CALLS} after a warm call),",
             f"# {ROUNDS} rounds alternating dory_halo_bf16_ghosts 0 / 1 under gcn_bf16_gather = 2 and dory_halo_bf16_rows = 1",
             "# width exact | wire row bytes | bytes written per row widening / keep | unpack ms widening (rounds) | unpack ms keep (rounds) | "
             "medians widening / keep, ratio | spread of widening | widen-on-download ms (one call) | verdict"]
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
            ctx.halo_bf16_rows(1)
            cur = w
        ctx.set_option("halo_exact_rows", exact)
        ld = ctx.info(0, "h", ptr=False)[2]
        rbuf = torch.rand(n * ld // 2, device="cuda")           # (as bf16 pairs: finite or not, both kernels only move bits)
        torch.cuda.synchronize()
        t = {0: [], 1: []}
        for _ in range(ROUNDS):
            for o in (0, 1):
                ctx.halo_bf16_ghosts(o)
                eb, re = ctx.halo_wire_row(1, da.FORWARD)
                assert eb == 2
                t[o].append(timed(ctx, ctx.halo_unpack, 1, da.FORWARD, rbuf.data_ptr()))
        # the dense widening: one call on a tensor whose twin alone is current (the last round left the switch on)
        ctx.halo_unpack(1, da.FORWARD, rbuf.data_ptr())
        ctx.sync()
        ctx.timing_reset()
        ctx.timing_enable(True)
        st = ctx.halo_bf16_ghosts_stats()["widened"]
        ctx.info(1, "fg")                           # dory_tensor_info hands the pointer out: the twin is widened first
        ctx.sync()
        wms, wn = ctx.timing_get("bf16_widen")
        ctx.timing_enable(False)
        assert wn == 1 and ctx.halo_bf16_ghosts_stats()["widened"] == st + 1
        ctx.halo_bf16_ghosts(0)
        med = {o: float(np.median(v)) for o, v in t.items()}
        spread = max(t[0]) - min(t[0])
        verdict = "keep not slower" if med[1] <= med[0] + 2 * spread else "keep SLOWER beyond twice the spread"
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        lines.append(f"{w} {exact} | {2 * re} | {4 * ld} / {2 * ld} | {fm(t[0])} | {fm(t[1])} | {med[0]:.4f} / {med[1]:.4f}, {med[1] / med[0]:.3f} | "
                     f"{spread:.4f} | {wms:.4f} | {verdict}")
        print(lines[-1], flush=True)
        del rbuf
        # (the raw pointer of fg@1 is out now: a fresh context for the next width keeps the TWIN state measurable)
        ctx.close()
        ctx, cur = None, None
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
