#!/usr/bin/env python3
"""What does the fused halo pack's row-wise form (dory_halo_fused_pack_rowwise) cost the producing kernel, against the pair it
replaces -- the plain producer plus the pack kernel of the wire format?  The four producers (tanh_backward -> g, tanh_forward -> h,
softmax + loss -> g of the last layer, the GAT prototype's softmax - label -> grad) on a synthetic partition (rank 0 of 8, every
local row listed for 1 peer, then for 3 peers), each shape in the padded fp32, exact fp32 and (padded) bf16 wire formats; device time
by events (the library's timing families):
  pair  the parent's: family "loss" of the producing call (for softmax + loss that includes the validation statistics' two
        kernels -- the same ones on both sides) plus family "halo" of dory_halo_pack into a device buffer (it follows the wire rule)
  send  the send form alone: family "loss" of the same call with dory_halo_fused_pack_rowwise on
ten timed calls after a warm one per measurement.  The pair is measured on the baseline library (--parent-lib: a build of the
commit before the switch; without it, this tree's library with the switch off), the send form on this tree's; the two libraries
alternate over ROUNDS rounds, baseline first.  Every step -- one shape, one library, one round: three wire formats at two fan-outs --
runs in a child process of its own under a time limit; the first step that fails or runs out of time ends the run.  After its
last measurement a send step sends the rows once and checks that the exchange counted them as written by a row-wise producer.
Needs no file outside the tree.  No link and no second GPU is involved: nothing here says anything about an exchange's transfer.
GPU box only:  python tools/halo_fused_rowwise_rate.py [--rows 1048576] [--parent-lib PATH] [--out FILE] [--step-timeout 150]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, CALLS, PEERS = 3, 10, 8
WIRES = ("padded", "exact", "bf16")
# name, model, dims(width), transform-first option, source tensor, inputs to fill, the producing call, (layer, dir) of the exchange
SHAPES = tuple(
    [(f"tanh_backward {w}", "GCN", [w + 8, w, 2], 2, (0, "g"), [(0, "aTg"), (0, "z")], ("apply_vertex", 0, 1), (0, 1)) for w in (128, 64, 48, 41)] +
    [(f"tanh_forward {w}", "GCN", [w + 8, w, 2], 1, (0, "h"), [(0, "z")], ("apply_vertex", 0, 0), (1, 0)) for w in (128, 64, 48, 41)] +
    [(f"softmax_xent {w}", "GCN", [w + 16, w + 8, w], 2, (1, "g"), [(1, "z")], ("apply_vertex", 1, 0), (1, 1)) for w in (41, 16, 64)] +
    [(f"softmax_sub {w}", "GAT", [4, 8, w], 0, (1, "grad"), [(1, "ah")], ("predict_gat", 2), (2, 1)) for w in (41, 16, 64)])
HEADER = "# shape | wire | peers per row | send rows | pair: producer + pack (rounds) | send producer (rounds) | medians pair / send | ratio | spread of the pair | verdict"


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


def one_step(n, si, send_side):
    """one shape on the library of this process: one line `wire per_row send_rows ms` per measurement"""
    import torch
    import dorylus_amd as da
    from halo_exact_rate import synthetic_partition
    name, model, dims, tf, src, inputs, call, (xl, xdir) = SHAPES[si]
    have = hasattr(da.load(), "dory_halo_fused_pack_rowwise")
    assert have or not send_side, "this library has no dory_halo_fused_pack_rowwise"
    ctx = da.Context(0)
    ctx.configure(getattr(da, model), dims, 3 * n, 0, PEERS)
    if tf:
        ctx.set_option("gcn_transform_first", tf)
    ctx.graph_upload(synthetic_partition(n))
    ctx.preallocate()
    if model == "GCN":
        assert ctx.transform_first_layer(src[0]), "the layer is not transform-first"
    ctx.labels_upload(np.random.default_rng(1).integers(0, dims[-1], n).astype(np.uint32))
    for k, (layer, nm) in enumerate(inputs):
        ctx.fill_uniform(layer, nm, k + 1, -2.0, 2.0)
    ctx.halo_fused_pack(1)
    sent = []
    ctx.set_host_transport(lambda s_, sc, so, r_, rc, ro: sent.append(int(sc.sum())), lambda buf: None)
    produce = getattr(ctx, call[0])
    sbuf = torch.empty(3 * n * ((dims[src[0] + 1] + 31) // 32 * 32) + 16, device="cuda")
    torch.cuda.synchronize()
    slots = [np.zeros(0, np.uint32)] + [x.astype(np.uint32) for x in np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)]
    own = np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)      # every row once (to the peer that owns its block), or to three peers
    for per_row in (1, 3):
        send = [np.zeros(0, np.uint32)] + [np.sort(np.concatenate([own[(q + k) % (PEERS - 1)] for k in range(per_row)])) for q in range(PEERS - 1)]
        send_rows = int(sum(len(x) for x in send))
        ctx.halo_plan(xdir, send, slots)
        for wire in WIRES:
            bf16 = wire == "bf16"
            ctx.set_option("halo_exact_rows", int(wire == "exact"))
            if model == "GCN":
                ctx.set_option("gcn_bf16_gather", 2 if bf16 else 0)
            else:
                ctx.gat_bf16_gather(2 if bf16 else 0)
            ctx.halo_bf16_rows(int(bf16))
            ctx.halo_fused_pack_bf16(int(bf16))
            eb, re = ctx.halo_wire_row(xl, xdir)
            assert eb == (2 if bf16 else 4), (wire, eb)
            if send_side:
                ctx.halo_fused_pack_rowwise(1)
                ms = timed(ctx, "loss", produce, *call[1:])
                before, nsent = ctx.halo_fused_pack_rowwise_stats(), len(sent)
                ctx.halo_exchange(xl, xdir)       # the rows the last call left travel: counted as a row-wise producer's
                ctx.sync()
                after = ctx.halo_fused_pack_rowwise_stats()
                assert (after[0] - before[0], after[1] - before[1]) == (1, send_rows) and sent[nsent:] == [send_rows * re * eb // 4], (before, after, sent[nsent:])
            else:
                if have:
                    ctx.halo_fused_pack_rowwise(0)
                ms = timed(ctx, "loss", produce, *call[1:]) + timed(ctx, "halo", ctx.halo_pack, xl, xdir, sbuf.data_ptr())
            print(f"STEP {wire} {per_row} {send_rows} {ms:.5f}", flush=True)
    del sbuf
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--parent-lib", default=None, help="the baseline library: a build of the commit before the switch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=150, help="seconds one step (one shape on one library) may take")
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)      # (the child: shape index, 0 pair / 1 send)
    a = ap.parse_args()
    if a.step:
        one_step(a.rows, *a.step)
        return 0
    base = os.path.abspath(a.parent_lib) if a.parent_lib else None
    lines = [f"# tools/halo_fused_rowwise_rate.py: {a.rows} local rows, rank 0 of {PEERS}; pair on {'the parent library' if base else 'the library of the tree, switch off'},",
             f"# send form on the library of the tree; ms per call (mean of {CALLS} after a warm call), {ROUNDS} rounds alternating the two; no link, one GPU", HEADER]
    print("\n".join(lines), flush=True)
    rc = 0
    for si in ([int(x) for x in a.shapes.split(",")] if a.shapes else range(len(SHAPES))):
        res = {}        # (wire, per_row) -> {"rows": .., 0: [pair per round], 1: [send per round]}
        for rnd in range(ROUNDS):
            for side in (0, 1):
                env = dict(os.environ)
                env.pop("DORY_LIB_PATH", None)
                if side == 0 and base:
                    env["DORY_LIB_PATH"] = base
                try:       # a fresh child process per step, under its own time limit; the first failure ends the run
                    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--rows", str(a.rows), "--step", str(si), str(side)],
                                       capture_output=True, text=True, timeout=a.step_timeout, env=env)
                except subprocess.TimeoutExpired:
                    lines.append(f"# STOPPED: {SHAPES[si][0]} ran longer than {a.step_timeout} s")
                    rc = 124
                    break
                if r.returncode != 0:
                    lines.append(f"# STOPPED: {SHAPES[si][0]} ended with status {r.returncode}\n# " + r.stderr.strip()[-1500:].replace("\n", "\n# "))
                    rc = r.returncode
                    break
                for ln in r.stdout.splitlines():
                    if ln.startswith("STEP "):
                        _, wire, per_row, rows, ms = ln.split()
                        e = res.setdefault((wire, int(per_row)), {"rows": int(rows), 0: [], 1: []})
                        e[side].append(float(ms))
            if rc:
                break
        if rc:
            print(lines[-1], flush=True)
            break
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        for per_row in (1, 3):
            for wire in WIRES:
                e = res[(wire, per_row)]
                mp, ms_, spread = float(np.median(e[0])), float(np.median(e[1])), max(e[0]) - min(e[0])
                verdict = ("cheaper than the pair" if ms_ <= mp - spread else "inside the pair's spread" if ms_ <= mp + spread
                           else "SLOWER than the producer plus the pack it replaces")
                lines.append(f"{SHAPES[si][0]} | {wire} | {per_row} | {e['rows']} | {fm(e[0])} | {fm(e[1])} | {mp:.4f} / {ms_:.4f} | x{ms_ / mp:.3f} | {spread:.4f} | {verdict}")
                print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
