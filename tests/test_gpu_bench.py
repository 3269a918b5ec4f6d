"""bench.py as the yardstick runs it: a plain run times exactly --steps steps and prints only the headline; --dump-outputs
writes what the last timed step left, the same arrays from run to run and from a --full run of the same arguments."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FULL_ONLY = ("roofline", "end_to_end", "to_patience_exit_lr1", "cpu_baseline", "parity_vs_cpu", "mean_abs_err_vs_truth")


def run_bench(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--workload", "C1", *args], cwd=ROOT,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def load(d):
    return {k: np.load(os.path.join(d, k + ".npy")) for k in ("S_vec", "obj", "avg")}


def test_bench_plain_and_full_dump_the_same_outputs(tmp_path):
    K, W = 7, 3
    a = run_bench("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "a"))
    assert a["steps"] == K and a["warmup"] == W and a["ms_per_step"] > 0
    assert a["value"] == pytest.approx(1e3 / a["ms_per_step"])
    assert a["metric"] == "DESC_PGD iters/sec" and a["unit"] == "iters/s" and a["higher_is_better"] is True and a["dtype"] == "f64"
    assert not any(k in a for k in FULL_ONLY)
    out = load(tmp_path / "a")
    assert all(x.dtype == np.float64 for x in out.values())
    assert out["S_vec"].shape == (a["config"]["m"],) and out["obj"].shape == out["avg"].shape == (W + K,)
    assert np.all((out["S_vec"] >= 0) & (out["S_vec"] <= 1))

    run_bench("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "b"))
    f = run_bench("--steps", str(K), "--warmup", str(W), "--dump-outputs", str(tmp_path / "f"), "--full")
    assert all(k in f for k in FULL_ONLY) and f["parity_vs_cpu"]["max_abs"] <= 1e-10
    for other in (load(tmp_path / "b"), load(tmp_path / "f")):
        for k in out:
            assert np.array_equal(out[k], other[k]), k
