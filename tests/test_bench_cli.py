"""bench.py's command line: a plain run prints the headline alone, ``--full`` adds the phase
breakdown, ``--dump-outputs`` writes the last timed generation's state, identically from run
to run.  Driven on the host (``--device cpu``, a tiny CMA-ES config)."""
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TINY = ["--device", "cpu", "--gpus", "1", "--pop", "32", "--dim", "12", "--steps", "3", "--warmup", "1"]


def _run(args):
    e = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_PORT"):
        e.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py")] + TINY + args, capture_output=True, text=True,
                       timeout=240, env=e, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def test_plain_and_full_runs_dump_the_same_outputs(tmp_path):
    plain = _run(["--dump-outputs", str(tmp_path / "a")])
    full = _run(["--full", "--phase-steps", "1", "--dump-outputs", str(tmp_path / "b")])
    for d in (plain, full):
        assert d["steps"] == 3 and d["warmup"] == 1
        assert d["ms_per_step"] > 0 and d["higher_is_better"] is True and d["dtype"] == "fp32"
        assert abs(d["value"] - 32 * 1e3 / d["ms_per_step"]) <= 1e-3 * d["value"]
    assert "phases_ms_eager" not in plain and "eigh_stats" not in plain
    assert set(full["phases_ms_eager"]) >= {"ask", "evaluate", "tell"}
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == sorted(os.listdir(tmp_path / "b"))
    assert {"algorithm.mean.npy", "algorithm.sigma.npy", "algorithm.C.npy", "algorithm.population.npy"} <= set(names)
    total = 0
    for n in names:
        a, b = np.load(tmp_path / "a" / n), np.load(tmp_path / "b" / n)
        assert a.dtype in (np.float32, np.float64) and np.isfinite(a).all(), n
        # the eager phase generations of --full run after the dump: same arguments, same arrays
        assert np.array_equal(a, b), n
        total += a.nbytes
    assert total <= 64 << 20
    assert np.load(tmp_path / "a" / "algorithm.population.npy").shape == (32, 12)


def test_dump_samples_rows_of_large_arrays(tmp_path):
    import torch

    sys.path.insert(0, ROOT)
    import bench
    from evoxmi.core import State

    big = torch.arange(5000 * 1000, dtype=torch.float32).reshape(5000, 1000)  # 20 MB
    st = State(small=torch.ones(3, dtype=torch.int64)).update_child("algorithm", State(big=big))
    bench.dump_outputs(st, str(tmp_path))
    got = np.load(tmp_path / "algorithm.big.npy")
    k = bench.DUMP_ARRAY_BYTES // 4000
    assert got.shape == (k, 1000) and got.dtype == np.float32
    rows = (got[:, 0] / 1000).astype(np.int64)
    assert (np.diff(rows) > 0).all() and np.array_equal(got, big.numpy()[rows])
    bench.dump_outputs(st, str(tmp_path / "again"))
    assert np.array_equal(got, np.load(tmp_path / "again" / "algorithm.big.npy"))
    small = np.load(tmp_path / "small.npy")
    assert small.dtype == np.float64 and small.tolist() == [1.0, 1.0, 1.0]
