"""bench.py's output contract (the driver parses this line): one JSON object on the last stdout line with the
metric fields, the roofline and (with --full) cpu_baseline objects; without a GPU the script must refuse, not fall back.
A plain run carries the headline only, and --dump-outputs writes what its last timed step computed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_bench_refuses_without_gpu():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--steps", "1", "--warmup", "0", "--scale", "0.001"],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0
    assert "no CPU fallback" in (r.stderr + r.stdout)


@pytest.mark.gpu
def test_bench_json_line_contract():
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--scale", "0.02", "--cpu-rows", "2000", "--full"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines            # stdout carries the JSON line and nothing else
    line = lines[0]
    d = json.loads(line)
    for k, t in (("metric", str), ("value", float), ("unit", str), ("n_gpus", int), ("steps", int), ("warmup", int),
                 ("ms_per_step", float), ("higher_is_better", bool), ("scaling", str), ("dtype", str), ("data", str),
                 ("config", dict)):
        assert isinstance(d[k], t), (k, d[k])
    assert d["n_gpus"] == 1 and d["steps"] == 2 and d["warmup"] == 1 and d["higher_is_better"] is True
    assert d["unit"] == "edges/s" and d["dtype"] == "f32" and d["data"] == "synthetic" and d["vs_baseline"] is None
    assert "workload" in d["config"] and "model" not in d["config"]
    assert d["value"] > 0 and d["ms_per_step"] > 0
    rf = d["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and rf["traffic"] is None    # PMC traffic only for the full-size run
    cb = d["cpu_baseline"]
    assert cb["kind"] == "port" and cb["cores"] >= 1 and cb["value"] > 0 and cb["unit"] == "edges/s" and cb["sample"]
    assert cb["gpu_vs_oracle_rel_err_ah0"] < 1e-4
    up = d["parity_unpinned"]     # what 1e-4 does not cover with reference-generated numbers, stated in the line itself
    assert isinstance(up, list) and len(up) == 5 and all(isinstance(x, str) for x in up)
    for word in ("gat edge ops", "maskout", "adam", "xavier", "gatmh"):
        assert any(word in x for x in up), word
    tf = d["transform_first"]
    assert tf is None or tf["ms_per_step"] > 0


def test_parity_unpinned_is_declared_without_a_gpu():
    sys.path.insert(0, ROOT)
    import bench
    assert len(bench.PARITY_UNPINNED) == 5 and any("gatmh" in x for x in bench.PARITY_UNPINNED)
    assert '"parity_unpinned": PARITY_UNPINNED' in open(os.path.join(ROOT, "bench.py")).read()


def test_multi_gpu_on_record_points_at_committed_evidence():
    sys.path.insert(0, ROOT)
    import bench
    rec = bench.multi_gpu_on_record()
    assert "not measured by this run" in rec["note"]
    assert rec["projected_epoch_ms"]["reddit:uniform"]["8"] > 0 and os.path.exists(os.path.join(ROOT, rec["projection_source"]))
    assert any(r["halo_overlap_fraction"] for r in rec["overlap_on_one_gpu"]) and all(r["identical_bits_overlap_on_off"] for r in rec["overlap_on_one_gpu"])


def test_stdout_is_shielded_while_communicators_are_created():
    """RCCL writes a line to file descriptor 1 when a communicator is created; bench.py points fd 1 at stderr for that time"""
    code = ("import os, sys; sys.path.insert(0, %r); import bench\n"
            "with bench.stdout_to_stderr():\n"
            "    os.write(1, b'noise from a library\\n')\n"
            "print('{\"json\": 1}')\n") % ROOT
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.strip() == '{"json": 1}' and "noise from a library" in r.stderr


def _bench(args, timeout=600):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + args, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.strip()]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_line_is_the_headline_and_dumps_its_last_step(tmp_path):
    """without --full nothing beside the headline runs; --dump-outputs writes the same arrays for the same arguments"""
    from helpers import rel_err
    import numpy as np
    dirs = [tmp_path / "a", tmp_path / "b"]
    runs = [_bench(["--gpus", "1", "--steps", "3", "--warmup", "1", "--scale", "0.02", "--dump-outputs", str(d)]) for d in dirs]
    for d in runs:
        assert d["steps"] == 3 and d["warmup"] == 1 and d["ms_per_step"] > 0 and d["unit"] == "edges/s" and d["dtype"] == "f32"
        assert d["higher_is_better"] is True and d["value"] > 0 and "GCN" in d["metric"]
        assert d["cpu_baseline"] is None and d["transform_first"] is None and d["cached_ah0"] is None
        for k in ("gat", "gatmh", "rmat", "community", "amazon_rank0of8", "friendster_rank0of8"):
            assert k not in d, k
    names = sorted(f.name for f in dirs[0].iterdir())
    assert names == sorted(["W0.npy", "W1.npy", "dW0.npy", "dW1.npy", "train_stat.npy", "rows.npy", "h0.npy", "logits.npy"]), names
    assert sum(f.stat().st_size for f in dirs[0].iterdir()) <= 64 << 20
    a = {n[:-4]: np.load(dirs[0] / n) for n in names}
    b = {n[:-4]: np.load(dirs[1] / n) for n in names}
    for n in a:
        assert a[n].dtype in (np.float32, np.float64) and np.isfinite(a[n]).all(), n
        assert a[n].shape == b[n].shape, n
    assert a["W0"].shape == (602, 128) and a["W1"].shape == (128, 41)
    assert a["h0"].shape == (a["rows"].size, 128) and a["logits"].shape == (a["rows"].size, 41)
    assert np.array_equal(a["rows"], b["rows"]) and a["train_stat"][2] > 0
    for n in a:
        assert rel_err(b[n], a[n]) < 1e-4, (n, rel_err(b[n], a[n]))


def test_dump_outputs_without_a_gpu(tmp_path):
    """dump_outputs against a stand-in context: names, dtypes, the seeded row sample and the size budget"""
    sys.path.insert(0, ROOT)
    import numpy as np
    import bench

    class Ctx:
        L = 2
        shapes = {(0, "h"): 128, (1, "z"): 41}

        def weight_get(self, l, name):
            return np.full((602, 128) if l == 0 else (128, 41), l + 1.0, np.float32)

        def weight_grad_get(self, l, name):
            return -self.weight_get(l, name)

        def train_stat(self):
            return 7.0, 3.5, 100

        def info(self, l, name):
            return N, self.shapes[(l, name)], 0, 0

        def download(self, l, name):
            return np.arange(N * self.shapes[(l, name)], dtype=np.float32).reshape(N, -1)

    N = 200000
    g = {"localVtxCnt": N, "localToGlobal": np.arange(N, dtype=np.uint32)[::-1] + 5}
    for d in (tmp_path / "a", tmp_path / "b"):
        bench.dump_outputs(Ctx(), g, "gcn", str(d))
    files = sorted(f.name for f in (tmp_path / "a").iterdir())
    assert files == sorted(["W0.npy", "W1.npy", "dW0.npy", "dW1.npy", "train_stat.npy", "rows.npy", "h0.npy", "logits.npy"])
    assert sum(f.stat().st_size for f in (tmp_path / "a").iterdir()) <= 64 << 20
    rows = np.load(tmp_path / "a" / "rows.npy")
    h0, lg = np.load(tmp_path / "a" / "h0.npy"), np.load(tmp_path / "a" / "logits.npy")
    assert rows.dtype == np.float64 and h0.dtype == np.float32 and 1000 < rows.size < N
    assert np.array_equal(rows, np.load(tmp_path / "b" / "rows.npy"))         # the sample is fixed
    local = (N + 4 - rows).astype(np.int64)                                    # back from the global ids above
    assert np.all(np.diff(local) > 0) and h0.shape == (rows.size, 128) and lg.shape == (rows.size, 41)
    assert np.array_equal(h0[:, 0], local * 128.0) and np.array_equal(lg[:, 0], local * 41.0)
    assert np.array_equal(np.load(tmp_path / "a" / "train_stat.npy"), [7.0, 3.5, 100.0])
    assert np.array_equal(np.load(tmp_path / "a" / "dW1.npy"), -np.load(tmp_path / "a" / "W1.npy"))
