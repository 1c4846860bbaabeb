"""bench.py on the GPU at a small size: a plain run times exactly --steps steps and writes what its last step computed;
--full adds the other seeds and the measurements beside the headline."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, D, K = 3000, 64, 8


def _bench(*extra):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "4", "--warmup", "1", "--N", str(N),
           "--D", str(D), "--k", str(K), *extra]
    r = subprocess.run(cmd, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    for key in ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step"):
        assert key in d, key
    assert d["metric"] == "settles/sec" and d["unit"] == "settles/s" and d["higher_is_better"] is True
    assert d["value"] == pytest.approx(1000.0 / d["ms_per_step"])
    return d


def test_plain_bench_times_the_steps_asked_for_and_dumps_the_last_step(tmp_path):
    from oscillink_amd import Oscillink

    d = _bench("--dump-outputs", str(tmp_path))
    assert d["steps_timed_total"] == 4 and d["config"]["seeds"] == [0] and d["full"] is False
    for key in ("cpu_baseline", "knn", "first_settle_ms", "receipt_ms"):
        assert key not in d, key
    U, rows = np.load(tmp_path / "U.npy"), np.load(tmp_path / "U_rows.npy")
    assert U.dtype == np.float32 and U.shape == (N, D) and np.array_equal(rows, np.arange(N))
    # the last timed step = reset_U + settle: the same as the first settle of a fresh lattice on the same inputs
    rng = np.random.default_rng(0)
    Y = rng.standard_normal((N, D)).astype(np.float32)
    psi = Y[:32].mean(axis=0)
    psi = (psi / (np.linalg.norm(psi) + 1e-12)).astype(np.float32)
    lat = Oscillink(Y, kneighbors=K, deterministic_k=False)
    lat.set_query(psi)
    st = lat.settle(dt=1.0, max_iters=12, tol=1e-3)
    assert np.load(tmp_path / "settle_iters.npy").tolist() == [float(st["iters"])]
    assert np.load(tmp_path / "settle_res.npy")[0] == pytest.approx(st["res"], rel=1e-3)
    assert float(np.linalg.norm(U - lat.U) / np.linalg.norm(lat.U)) < 1e-5
    lat.close()


def test_full_bench_adds_the_other_seeds_and_measurements():
    d = _bench("--full")
    assert d["full"] is True and d["config"]["seeds"] == [0, 1, 2] and d["steps_timed_total"] == 12
    for key in ("cpu_baseline", "knn", "first_settle_ms", "mispredict_settle_ms", "ustar_solve_ms", "receipt_ms"):
        assert key in d, key
