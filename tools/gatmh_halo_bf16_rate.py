#!/usr/bin/env python3
"""What do the kernels of dory_gatmh_halo_bf16 cost on the device, against their fp32 siblings?  The 8-head GAT's backward sweep on a
synthetic partition (rank 0 of 8, every local row listed for 1 peer, then for 3 peers), layer shapes (K, D) = (8, 16), (4, 16) and
(4, 64) as hidden layers and (1, 41) as a last layer, padded and exact wire; device time by events (the library's timing families):
  produce  fp32: family "loss" of the whole backward dory_aggregate with dory_gatmh_bwd_merged_exchange and dory_halo_fused_pack on
                 (the ELU backward / head expansion, then gatmh_dst_rowwise_send_kernel; no pack kernel runs)
           bf16: the same with dory_halo_bf16_rows, dory_gatmh_halo_bf16 and gatmh_bf16_gather = 2 on top
                 (gatmh_dst_rowwise_send_bf16_kernel) -- the exchange goes through a host transport that moves nothing and is not part
                 of any number here, and neither is the source side (families "spmm", "bf16_convert")
  pack     fp32: dory_gatmh_bwd_pack (gather_rows_pair_kernel);  bf16: the same call under the rule (gather_rows_pair_bf16_kernel)
  unpack   fp32: dory_gatmh_bwd_unpack (scatter_rows_pair_kernel);  bf16: the same call (scatter_rows_pair_bf16_kernel)
ten timed calls after a warm one per measurement.  The fp32 forms are measured on the baseline library (--parent-lib: a build of the
commit before the switch; without it, this tree's library with the switch off), the bf16 forms on this tree's; the two libraries
alternate over ROUNDS rounds, baseline first.  Every step -- one shape, one library, one round -- runs in a child process of its own
under a time limit; the first step that fails or runs out of time ends the run; what has been measured by then is written out.  A
bf16 produce step checks after its last measurement that the exchanges were counted as producer-packed bf16 ones.  Needs no file
outside the tree.  No link and no second GPU is involved: nothing here says anything about an exchange's transfer -- the byte counts
per row are arithmetic.
GPU box only:  python tools/gatmh_halo_bf16_rate.py [--rows 1048576] [--parent-lib PATH] [--out FILE] [--step-timeout 300]"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
ROUNDS, CALLS, PEERS = 3, 10, 8
WIRES = ("padded", "exact")
# name, dims, heads, the measured layer
SHAPES = (("hidden 8 x 16", [8, 128, 4], [8, 1], 0), ("hidden 4 x 16", [8, 64, 4], [4, 1], 0), ("hidden 4 x 64", [8, 256, 4], [4, 1], 0),
          ("last 1 x 41", [8, 16, 41], [2, 1], 1))
KINDS = ("produce", "pack", "unpack")
HEADER = "# shape | wire | peers per row | send rows | row floats fp32 -> bf16 | what | fp32 (rounds) | bf16 (rounds) | medians fp32 / bf16 | ratio | spread of the fp32 form | verdict"


def timed(ctx, families, fn):
    fn()
    ctx.sync()
    ctx.timing_reset()
    ctx.timing_enable(True)
    for _ in range(CALLS):
        fn()
    ctx.sync()
    ms = 0.0
    for fam in families:
        t, n = ctx.timing_get(fam)
        assert n and n % CALLS == 0, (fam, n)
        ms += t
    ctx.timing_enable(False)
    return ms / CALLS


def one_step(n, si, new_side):
    """one shape on the library of this process: one line `STEP wire per_row send_rows row_pair row_merged kind ms` per measurement"""
    import torch
    import dorylus_amd as da
    from halo_exact_rate import synthetic_partition
    name, dims, heads, layer = SHAPES[si]
    have = hasattr(da.load(), "dory_gatmh_halo_bf16")
    assert have or not new_side, "this library has no dory_gatmh_halo_bf16"
    K = heads[layer]
    zw = dims[layer + 1] * (K if layer == 1 else 1)
    pad = lambda c: (c + 31) // 32 * 32
    ctx = da.Context(0)
    ctx.configure(da.GATMH, dims, 3 * n, 0, PEERS)
    ctx.gatmh_heads(heads)
    ctx.graph_upload(synthetic_partition(n))
    ctx.preallocate()
    if new_side:          # (the forward sweeps gather rounded rows too: every layer of these shapes takes the sweep forms)
        ctx.set_option("gatmh_bf16_gather", 2)
        ctx.halo_bf16_rows(1)
        ctx.gatmh_halo_bf16(1)
    rng = np.random.default_rng(1)
    ctx.labels_upload(rng.integers(0, dims[-1], n).astype(np.uint32))
    ctx.fill_uniform(0, "h", 1, -1.0, 1.0)
    widths = [dims[1], dims[2] * heads[1]]
    for l in range(2):
        fi = dims[0] if l == 0 else widths[0]
        ctx.weight_set(l, "w", (rng.standard_normal((fi, widths[l])) / np.sqrt(fi)).astype(np.float32))
        ctx.weight_set(l, "a_l", (rng.standard_normal(widths[l]) * 0.3).astype(np.float32))
        ctx.weight_set(l, "a_r", (rng.standard_normal(widths[l]) * 0.3).astype(np.float32))
    calls = []
    ctx.set_host_transport(lambda s_, sc, so, r_, rc, ro: calls.append(int(sc.sum())), lambda buf: None)
    slots = [np.zeros(0, np.uint32)] + [x.astype(np.uint32) for x in np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)]
    own = np.array_split(np.arange(n, dtype=np.uint32), PEERS - 1)
    one_peer = [np.zeros(0, np.uint32)] + [own[q] for q in range(PEERS - 1)]
    for d in (da.FORWARD, da.BACKWARD):
        ctx.halo_plan(d, one_peer, slots)
    for l in range(layer + 1):                     # the forward pass up to the measured layer: its sweep form leaves op / dpos
        ctx.apply_vertex(l, da.FORWARD)
        ctx.halo_exchange(l + 1, da.FORWARD)
        ctx.apply_edge(l + 1, da.FORWARD)
        ctx.aggregate(l + 1, da.FORWARD)
    if layer == 1:
        ctx.predict_gat(2)
    else:
        ctx.fill_uniform(1, "dh", 3, -1.0, 1.0)
    ctx.sync()
    buf = torch.empty(3 * n * (pad(zw) + 4 * K) + 16, device="cuda")
    rbuf = torch.rand(n * (pad(zw) + pad(4 * K)) + 16, device="cuda")
    torch.cuda.synchronize()
    bwd = lambda: ctx.aggregate(layer + 1, da.BACKWARD)
    for per_row in (1, 3):
        send = [np.zeros(0, np.uint32)] + [np.sort(np.concatenate([own[(q + k) % (PEERS - 1)] for k in range(per_row)])) for q in range(PEERS - 1)]
        send_rows = int(sum(len(x) for x in send))
        ctx.halo_plan(da.BACKWARD, send, slots)
        for wire in WIRES:
            exact = int(wire == "exact")
            ctx.set_option("halo_exact_rows", exact)
            row_pair = ((zw + 3) // 4 * 4 if exact else pad(zw)) + 4 * K
            row_merged = ((zw + 7) // 8 * 8 if exact else pad(zw)) // 2 + 4 * K
            ms = {}
            assert ctx.gatmh_bwd_wire_row(layer)[0] == (row_merged if new_side else row_pair)
            ctx.set_option("gatmh_bwd_phase", 0)
            ctx.halo_fused_pack(1)
            ctx.gatmh_bwd_merged_exchange(1)
            before, ncalls = ctx.gatmh_bwd_merged_exchange_stats(), len(calls)
            b16 = ctx.gatmh_halo_bf16_stats() if new_side else None
            ms["produce"] = timed(ctx, ("loss",), bwd)
            after = ctx.gatmh_bwd_merged_exchange_stats()
            assert after[0] - before[0] == after[2] - before[2] == CALLS + 1 and after[3] == before[3], (before, after)
            assert calls[ncalls:] == [send_rows * (row_merged if new_side else row_pair)] * (CALLS + 1), calls[ncalls:][:3]
            if new_side:
                a16 = ctx.gatmh_halo_bf16_stats()
                assert a16[1] - b16[1] == a16[3] - b16[3] == CALLS + 1, (b16, a16)
            ctx.gatmh_bwd_merged_exchange(0)
            ctx.halo_fused_pack(0)
            ms["pack"] = timed(ctx, ("halo",), lambda: ctx.gatmh_bwd_pack(layer, buf.data_ptr()))
            ms["unpack"] = timed(ctx, ("halo",), lambda: ctx.gatmh_bwd_unpack(layer, rbuf.data_ptr()))
            for kind in KINDS:
                print(f"STEP {wire} {per_row} {send_rows} {row_pair} {row_merged} {kind} {ms[kind]:.5f}", flush=True)
    del buf, rbuf
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 20)
    ap.add_argument("--parent-lib", default=None, help="the baseline library: a build of the commit before the switch")
    ap.add_argument("--out", default=None)
    ap.add_argument("--step-timeout", type=int, default=300, help="seconds one step (one shape on one library) may take")
    ap.add_argument("--shapes", default=None, help="comma-separated indices into SHAPES (default: all)")
    ap.add_argument("--step", type=int, nargs=2, default=None, help=argparse.SUPPRESS)      # (the child: shape index, 0 pair / 1 new)
    a = ap.parse_args()
    if a.step:
        one_step(a.rows, *a.step)
        return 0
    base = os.path.abspath(a.parent_lib) if a.parent_lib else None
    lines = [f"# tools/gatmh_halo_bf16_rate.py: {a.rows} local rows, rank 0 of {PEERS}; fp32 forms on {'the parent library' if base else 'the library of the tree, switch off'},",
             f"# bf16 forms on the library of the tree; ms per call (mean of {CALLS} after a warm call), {ROUNDS} rounds alternating the two; ONE GPU, NO LINK, NO SECOND GPU",
             "# produce: ELU backward / head expansion + gatmh_dst_rowwise_send[_bf16]_kernel; pack: gather_rows_pair[_bf16]_kernel; unpack: scatter_rows_pair[_bf16]_kernel",
             HEADER]
    print("\n".join(lines), flush=True)
    rc = 0
    for si in ([int(x) for x in a.shapes.split(",")] if a.shapes else range(len(SHAPES))):
        res = {}        # (wire, per_row, kind) -> {"rows": .., "row": (pair, merged), 0: [pair per round], 1: [new per round]}
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
                        _, wire, per_row, rows, rp, rm, kind, ms = ln.split()
                        e = res.setdefault((wire, int(per_row), kind), {"rows": int(rows), "row": (int(rp), int(rm)), 0: [], 1: []})
                        e[side].append(float(ms))
            if rc:
                break
        if rc:
            print(lines[-1], flush=True)
            break
        fm = lambda xs: " ".join(f"{x:.4f}" for x in xs)
        for kind in KINDS:
            for per_row in (1, 3):
                for wire in WIRES:
                    e = res[(wire, per_row, kind)]
                    mp, mn, spread = float(np.median(e[0])), float(np.median(e[1])), max(e[0]) - min(e[0])
                    verdict = "faster" if mn < mp - spread else "a tie (inside the fp32 form's spread)" if mn <= mp + spread else "NOT FASTER than its fp32 sibling"
                    lines.append(f"{SHAPES[si][0]} | {wire} | {per_row} | {e['rows']} | {e['row'][0]} -> {e['row'][1]} | {kind} | {fm(e[0])} | {fm(e[1])} | "
                                 f"{mp:.4f} / {mn:.4f} | x{mn / mp:.3f} | {spread:.4f} | {verdict}")
                    print(lines[-1], flush=True)
        if a.out:          # (after every shape: a run that is stopped leaves what it measured)
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write("\n".join(lines) + "\n")
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    return rc


if __name__ == "__main__":
    sys.exit(main())
