#!/usr/bin/env python3
"""What do the scatter-message kernels (dory_scatter_msgs_pack, and the unpack behind dory_scatter_msgs_deliver, through
dory_scatter_msgs_unpack on records that are on the device already) cost against the padded and the exact-width pack / unpack
(K6) for the same rows?  Device time only (timing family "halo"): no staging copy, no host, no link and no reference peer is
measured.  One context per width on the synthetic partition of tools/halo_exact_rate.py (rank 0 of 8, about 1 M send rows in
seven sorted per-peer lists with repeats across peers, 1 M ghost rows), the three forms alternating, ten timed calls after a warm
one per measurement, three rounds: the spread between the repeated measurements of one form is the yardstick's own noise.  The
messages are the reference's size (1 MiB).  Bytes moved per row: padded 4 (ld + ld), exact 4 (ld + cols), messages
4 (ld + cols + 1), and on the unpack a binary search of the id table per record.
GPU box only:  python tools/scatter_msgs_rate.py [--rows 1048576] [--out FILE]"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from halo_exact_rate import CALLS, PEERS, ROUNDS, synthetic_partition  # noqa: E402

WIDTHS = (41, 48, 128, 602)
FORMS = ("padded", "exact", "msgs")


def timed(ctx, fn):
    fn()
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(CALLS):
        fn()
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
    l2g = np.arange(n, dtype=np.uint32)
    src_gv = (n + 3 * np.arange(n)).astype(np.uint32)            # ascending, with holes: the search has something to do
    dst_gv = (4 * n + np.arange(n)).astype(np.uint32)
    lines = [f"# tools/scatter_msgs_rate.py: {send_rows} send rows, {n} ghost rows, rank 0 of {PEERS}; device ms per call (mean of {CALLS} after a warm call,",
             f"# timing family halo), {ROUNDS} rounds alternating the padded rows, the exact-width rows (halo_exact_rows) and the scatter messages (1 MiB each).",
             "# No staging copy, no link and no reference peer is measured.",
             "# width ld | bytes per row padded / exact / msgs | pack ms padded (rounds) | pack ms exact (rounds) | pack ms msgs (rounds) | "
             "unpack ms padded (rounds) | unpack ms exact (rounds) | unpack ms msgs (rounds) | medians pack p / e / m | medians unpack p / e / m | "
             "msgs / exact pack, unpack | spread of the exact form (max - min over the rounds) pack, unpack"]
    for w in WIDTHS:
        ctx = da.Context(0)
        ctx.configure(da.GCN, [4, w, 2], 5 * n, 0, PEERS)
        ctx.graph_upload(g)
        ctx.preallocate()
        ctx.halo_plan(da.FORWARD, send, slots)
        ctx.halo_wire_ids(l2g, src_gv, dst_gv)
        ctx.fill_uniform(0, "h", 1, -1.0, 1.0)
        ld = ctx.info(0, "h")[2]
        sbuf = torch.empty(send_rows * ld, device="cuda")
        rbuf = torch.rand(n * ld, device="cuda")
        msgs, total = ctx.scatter_msgs_layout(1, da.FORWARD)
        mbuf = torch.empty(total + 16, dtype=torch.uint8, device="cuda")
        # the records as seven peers send them: each peer's ghosts in ascending id, the peers one after the other
        rec = torch.rand(n, 1 + w, device="cuda").view(torch.int32)
        rec[:, 0] = torch.from_numpy(src_gv.astype(np.int32)).cuda()
        torch.cuda.synchronize()

        def msgs_unpack():
            ctx.scatter_msgs_unpack(1, da.FORWARD, rec.data_ptr(), n)
            assert ctx.scatter_msgs_finish(1, da.FORWARD) == (n, 0, 0)      # (the round ends outside the timed interval)

        t = {(k, f): [] for k in ("pack", "unpack") for f in FORMS}
        for _ in range(ROUNDS):
            for f in FORMS:
                if f == "msgs":
                    t[("pack", f)].append(timed(ctx, lambda: ctx.scatter_msgs_pack(1, da.FORWARD, mbuf.data_ptr())))
                    t[("unpack", f)].append(timed(ctx, msgs_unpack))
                else:
                    ctx.set_option("halo_exact_rows", 1 if f == "exact" else 0)
                    t[("pack", f)].append(timed(ctx, lambda: ctx.halo_pack(1, da.FORWARD, sbuf.data_ptr())))
                    t[("unpack", f)].append(timed(ctx, lambda: ctx.halo_unpack(1, da.FORWARD, rbuf.data_ptr())))
        med = {k: float(np.median(v)) for k, v in t.items()}
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        spread = lambda k: max(t[(k, "exact")]) - min(t[(k, "exact")])
        lines.append(f"{w} {ld} | {8 * ld} / {4 * (ld + w)} / {4 * (ld + w + 1)} | " + " | ".join(fm(t[(k, f)]) for k in ("pack", "unpack") for f in FORMS) +
                     f" | {med[('pack', 'padded')]:.4f} / {med[('pack', 'exact')]:.4f} / {med[('pack', 'msgs')]:.4f}"
                     f" | {med[('unpack', 'padded')]:.4f} / {med[('unpack', 'exact')]:.4f} / {med[('unpack', 'msgs')]:.4f}"
                     f" | {med[('pack', 'msgs')] / med[('pack', 'exact')]:.3f}, {med[('unpack', 'msgs')] / med[('unpack', 'exact')]:.3f}"
                     f" | {spread('pack'):.4f}, {spread('unpack'):.4f}")
        print(lines[-1], flush=True)
        del sbuf, rbuf, mbuf, rec
        ctx.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    print(text)


if __name__ == "__main__":
    main()
