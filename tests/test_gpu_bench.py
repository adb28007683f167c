"""-m gpu: bench.py on one GPU at a small shape -- a plain run prints the headline line only (the roofline leg and the CPU baseline
are --full extras), and --dump-outputs writes what the last timed step returned, the same files for the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M, N, K = 16384, 2048, 64


def _bench(*extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--m", str(M), "--n", str(N), "--k", str(K), *extra]
    res = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    lines = [ln for ln in res.stdout.splitlines() if ln.startswith("{")]
    assert res.returncode == 0 and len(lines) == 1, res.stdout[-1500:] + res.stderr[-3000:]
    return json.loads(lines[0])


def test_bench_plain_run_and_dumped_outputs(tmp_path):
    d1, d2 = tmp_path / "a", tmp_path / "b"
    out = _bench("--dump-outputs", str(d1))
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in out, key
    assert out["steps"] == 3 and out["value"] > 0 and out["ms_per_step"] > 0 and out["config"]["k_out"] == K
    assert "roofline" not in out and "cpu_baseline" not in out
    _bench("--dump-outputs", str(d2))
    names = sorted(p.name for p in d1.iterdir())
    assert names == ["S.npy", "U_rows.npy", "V.npy"]
    assert sum((d1 / nm).stat().st_size for nm in names) <= 64 * 2**20
    S, V, U = (np.load(d1 / nm) for nm in ("S.npy", "V.npy", "U_rows.npy"))
    assert S.shape == (K,) and V.shape == (N, K) and U.shape == (M, K)
    assert all(a.dtype == np.float64 for a in (S, V, U))
    assert np.all(np.diff(S) <= 0) and S[-1] > 0
    assert np.linalg.norm(V.T @ V - np.eye(K)) < 1e-9 and np.linalg.norm(U.T @ U - np.eye(K)) < 1e-9
    for nm in names:
        assert np.array_equal(np.load(d1 / nm), np.load(d2 / nm)), nm
