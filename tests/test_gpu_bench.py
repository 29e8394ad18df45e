"""bench.py under the DRIVER's flags (--steps 20 --warmup 5): the short window must measure the loop, not
start-up.  `value` is the 20 steps behind the warm-up; --full adds a window of whole check periods (the reference's
check schedule), and both agree with the sum of the in-loop kernel times (what rocprofv3 --kernel-trace reports for
the launches of a trial).  --dump-outputs writes the solver state after the last timed step, the same in every run."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_driver_flags_measure_the_steady_loop():
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                          "--cpu-iters", "0", "--kernels", "--full"], capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert out.returncode == 0, out.stderr[-2000:]
    rec = json.loads(out.stdout.strip().splitlines()[-1])
    assert rec["steps"] == 20 and rec["warmup"] == 5 and rec["n_gpus"] == 1
    # `value` and `ms_per_step` are the K = 20 steps the flags ask for (iterations 45..65: no check falls into them)
    assert rec["timed_window"] == "iterations 45..65" and rec["timed_steps"] == 20 and rec["checks"] == 0
    assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]
    # --full: a window of whole 40-iteration check periods carries the reference's check schedule; the K steps may
    # only be a little faster than it, never slower than 10 % below it
    wp = rec["whole_check_periods"]
    assert wp["window"] == "iterations 80..480" and wp["iters"] == 400 and wp["checks"] == wp["iters"] // 40
    assert abs(wp["value"] - 1e3 / wp["ms_per_step"]) < 1e-6 * wp["value"]
    assert 0.90 * wp["value"] <= rec["value"] <= 1.20 * wp["value"], (rec["value"], wp["value"])
    # the launches of a trial, timed in the loop, add up to the step time within 15 % (2 launches when the trial is
    # fused — the A' y kernel then holds the decision and the next primal step —, else 3)
    k = rec["roofline"]["other_kernels_ms"]
    trial = k["spmv_ax_dual"] + k["spmv_aty_interact"] + (0.0 if rec["trial_launches"] == 2 else rec["kernels_ms"]["decide_primal"])
    assert abs(wp["ms_per_step"] - trial) <= 0.15 * wp["ms_per_step"], (wp["ms_per_step"], trial)
    r = rec["roofline"]
    assert abs(r["achieved"] - r["algorithmic_bytes_per_launch"] / (r["avg_launch_ms"] * 1e-3) / 1e9) < 1e-6 * r["achieved"]
    assert rec["startup_ms_first_40"] > 0 and rec["setup_seconds"] > 0


def test_plain_run_times_the_steps_and_dumps_the_same_outputs(tmp_path):
    """A plain run times exactly --steps steps behind the warm-up and prints the headline only; --dump-outputs writes
    the iterates after the last timed step, float64, and two runs with the same flags write the same arrays."""
    recs = []
    for k in range(2):
        d = tmp_path / ("run%d" % k)
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--config", "a", "--steps", "120",
                              "--warmup", "40", "--dump-outputs", str(d)], capture_output=True, text=True, timeout=300, cwd=ROOT)
        assert out.returncode == 0, out.stderr[-2000:]
        rec = json.loads(out.stdout.strip().splitlines()[-1])
        assert rec["timed_steps"] == 120 and rec["timed_window"] == "iterations 80..200"
        assert abs(rec["value"] - 1e3 / rec["ms_per_step"]) < 1e-6 * rec["value"]
        assert "roofline" not in rec and "cpu_baseline" not in rec and "whole_check_periods" not in rec
        recs.append(d)
    n, m = rec["config"]["n"], rec["config"]["m"]
    names = sorted(os.listdir(recs[0]))
    assert names == ["steps.npy", "x.npy", "x_avg.npy", "y.npy", "y_avg.npy"]
    for name in names:
        a, b = np.load(recs[0] / name), np.load(recs[1] / name)
        assert a.dtype == np.float64 and np.isfinite(a).all(), name
        assert a.shape == {"steps.npy": (8,), "x.npy": (n,), "x_avg.npy": (n,), "y.npy": (m,), "y_avg.npy": (m,)}[name], name
        assert np.array_equal(a, b), name
    assert np.abs(np.load(recs[0] / "x.npy")).max() > 0
