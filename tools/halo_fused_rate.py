#!/usr/bin/env python3
"""What does the fused halo pack (dory_halo_fused_pack) cost the producing GEMM, against the pack kernel it removes?  One context per
shape on a synthetic partition (rank 0 of 8, every local row listed for 1 peer, then for 3 peers), device time by events (the
library's timing families): per shape
  (a) the producer with the feature off      (family "gemm" of one dory_apply_vertex: the product that travels and, for the NT
                                              shape, the two other GEMMs of that call -- the same ones in (a) and (c))
  (b) the pack kernel alone                  (family "halo" of dory_halo_pack_tensor into a device buffer)
  (c) the producer with the feature on
ten timed calls after a warm one per measurement, ROUNDS alternations of off / on: (c) - (a) stands beside (b), with the spread of
the repeated (a) as the yardstick's own noise.  With a library from before the feature (DORY_LIB_PATH) only (a) and (b) are
measured: alternate such runs with these to see that the feature-off GEMM did not move.  Needs no file outside the tree.
GPU box only:  python tools/halo_fused_rate.py [--rows 1048576] [--out FILE]"""
import argparse
import os
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
    ("NN 128->41 padded", "GAT", [128, 41, 2], (0, "z"), (0, "h"), (0, 0), 0, 0),
    ("NN 128->41 exact", "GAT", [128, 41, 2], (0, "z"), (0, "h"), (0, 0), 0, 1),
)


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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import dorylus_amd as da
    from halo_exact_rate import synthetic_partition
    n = a.rows
    g = synthetic_partition(n)
    rng = np.random.default_rng(0)
    have = hasattr(da.load(), "dory_halo_fused_pack")
    slots = [np.zeros(0, np.uint32)] + [x.astype(np.uint32) for x in np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)]
    lines = [f"# tools/halo_fused_rate.py: {n} local rows, rank 0 of {PEERS}, library {da.LIB_PATH} ({'with' if have else 'WITHOUT'} the fused pack);",
             f"# ms per call (mean of {CALLS} after a warm call), {ROUNDS} rounds alternating off / on",
             "# shape | peers per row | send rows | packed MB | (a) producer off (rounds) | (c) producer on (rounds) | (b) pack kernel (rounds) |"
             " medians a / c / b | c - a | spread of a | verdict"]
    for name, model, dims, src, inp, prod, xdir, exact in SHAPES:
        for per_row in (1, 3):
            # every row once (to the peer that owns its block), or to three peers
            own = np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)
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
            sent = []
            ctx.set_host_transport(lambda s_, sc, so, r_, rc, ro: sent.append(int(sc.sum())), lambda buf: None)
            _, cols, ld, _ = ctx.info(src[0], src[1], ptr=False) if have else ctx.info(src[0], src[1])
            w = cols if exact else ld
            sbuf = torch.empty(send_rows * ld, device="cuda")
            torch.cuda.synchronize()
            t = {"a": [], "b": [], "c": []}
            for _ in range(ROUNDS):
                if have:
                    ctx.halo_fused_pack(0)
                t["a"].append(timed(ctx, "gemm", ctx.apply_vertex, *prod))
                t["b"].append(timed(ctx, "halo", ctx.halo_pack_tensor, src[0], src[1], xdir, sbuf.data_ptr()))
                if have:
                    ctx.halo_fused_pack(1)
                    t["c"].append(timed(ctx, "gemm", ctx.apply_vertex, *prod))
            if have and per_row == 1:      # and the rows the last producer left are the ones that travel: one exchange, counted as fused
                ctx.halo_exchange(1, xdir)
                ctx.sync()
                assert ctx.halo_fused_pack_stats()[:2] == (1, send_rows) and sent == [send_rows * w], (ctx.halo_fused_pack_stats(), sent)
            fm = lambda xs: " ".join(f"{x:.4f}" for x in xs) if xs else "-"
            ma, mb = float(np.median(t["a"])), float(np.median(t["b"]))
            spread = max(t["a"]) - min(t["a"])
            if have:
                mc = float(np.median(t["c"]))
                verdict = "cheaper than the pack" if mc - ma <= mb else "NOT recommended here: costs more than the pack it removes"
                tail = f"{ma:.4f} / {mc:.4f} / {mb:.4f} | {mc - ma:+.4f} | {spread:.4f} | {verdict}"
            else:
                tail = f"{ma:.4f} / - / {mb:.4f} | - | {spread:.4f} | -"
            lines.append(f"{name} | {per_row} | {send_rows} | {send_rows * w * 4 / 1e6:.1f} | {fm(t['a'])} | {fm(t['c'])} | {fm(t['b'])} | {tail}")
            print(lines[-1], flush=True)
            del sbuf
            ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
