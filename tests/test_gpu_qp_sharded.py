"""QPs whose Hessian has off-diagonal entries, row-block sharded over several GPUs.  N, the off-diagonal part of
Q, adds a third SpMV N x+ and the |dx . N dx| / 2 term of the step-size rule to every trial.  In the mesh layout rank g holds
the rows [c0, c1) of N, gathers from the all-gathered x+ and sums its dx . N dx partials as a fourth scalar of the decision's
exchange; with the RCCL exchange every rank keeps the whole N.  Every rank must hold the same bits, and the sharded solve
must reach the reference optimum of the single-GPU one.

The ranks are folded onto this one device (one thread per rank in a process, or one process per rank)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from highs_amd import solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLD = os.path.join(HERE, "golden")
REF_SPARSE = json.load(open(os.path.join(GOLD, "reference_qp_sparse.json")))
# (every one of them restarts on one GPU: 4 to 11 restarts in 40 to 440 iterations)
GOLDENS = ["sq0", "sq3", "sq7", "sq100", "sq102", "qjh_mps"]
FOLD_ENV = {"PDLP_MI355X_FOLD_DEVICES": "1", "PDLP_MI355X_VERIFY_RANKS": "1", "GPU_MAX_HW_QUEUES": "16"}


def _qp(name):
    return L.HighsLp.from_npz(os.path.join(GOLD, "qp", name + ".npz"))


_IN_PROCESS = r"""
import json, os, sys
sys.path.insert(0, %(root)r)
from highs_amd import solver, lp as L
out = {}
for name in %(names)r:
    lp = L.HighsLp.from_npz(os.path.join(%(gold)r, 'qp', name + '.npz'))
    r = solver.solveLpCupdlp(lp, kkt_tolerance=1e-8, pdlp_iteration_limit=400000, num_devices=%(world)d)
    err = solver.lib().pdlp_mi355x_last_error().decode(errors='replace') if r.model_status != solver.kOptimal else ''
    out[name] = dict(status=int(r.model_status), err=err, obj=r.info.get('objective_function_value'),
                     dres=r.info.get('max_dual_residual_error'), pdobj=r.info.get('primal_dual_objective_error'),
                     restarts=int(r.result.num_restarts), iters=int(r.pdlp_iteration_count))
print('RESULT ' + json.dumps(out))
"""


@pytest.mark.parametrize("world", [2, 4])
def test_sparse_hessian_qps_solve_sharded_in_process(world):
    """num_devices = world in one process (one host thread per rank, folded onto this device); PDLP_MI355X_VERIFY_RANKS
    makes the library compare every rank's solution bit for bit."""
    code = _IN_PROCESS % dict(root=ROOT, gold=GOLD, names=GOLDENS, world=world)
    env = dict(os.environ, **FOLD_ENV)
    p = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=900, env=env)
    assert p.returncode == 0, p.stdout[-2000:] + p.stderr[-2000:]
    line = [s for s in p.stdout.splitlines() if s.startswith("RESULT ")]
    assert line, p.stdout[-2000:] + p.stderr[-2000:]
    res = json.loads(line[-1][len("RESULT "):])
    for name in GOLDENS:
        r = res[name]
        assert r["status"] == solver.kOptimal, (name, r["err"])
        ref = REF_SPARSE[name]["objective_value"]
        assert abs(r["obj"] - ref) <= 1e-6 * (1 + abs(ref)), (name, r["obj"], ref)
        assert r["dres"] < 1e-6 and r["pdobj"] < 1e-6, (name, r)
        assert r["restarts"] > 0, name


def _run_ranks(world, case, tmp_path, extra_env=None):
    uid = (C.c_ubyte * 128).from_buffer_copy(os.urandom(128))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **FOLD_ENV)
    env.update(extra_env or {})
    tmp_path.mkdir(parents=True, exist_ok=True)
    outs = [str(tmp_path / f"r{r}.npz") for r in range(world)]
    procs = [subprocess.Popen(["timeout", "-k", "10", "300", sys.executable, os.path.join(HERE, "qp_mesh_worker.py"), str(r),
                               str(world), bytes(uid).hex(), case, outs[r]], env=env,
                              stdout=subprocess.PIPE, stderr=subprocess.STDOUT) for r in range(world)]
    logs = [p.communicate(timeout=360)[0].decode(errors="replace") for p in procs]
    for r, p in enumerate(procs):
        assert p.returncode == 0, f"rank {r} failed:\n{logs[r][-2000:]}"
    return [dict(np.load(o)) for o in outs]


_SOLVE_KEYS = ("col_value", "col_dual", "row_value", "row_dual", "num_iter", "num_trials", "num_restarts", "primal_obj",
               "dual_obj", "term")


@pytest.mark.parametrize("world", [2, 4])
@pytest.mark.parametrize("name", ["sq0", "sq102"])
def test_sparse_hessian_qp_solves_over_rank_processes(name, world, tmp_path):
    """One process per rank through pdlp_mi355x_create_sharded: the mesh exchange, one more launch per trial and per check."""
    res = _run_ranks(world, f"solve:{name}", tmp_path)
    for r in res[1:]:
        for k in _SOLVE_KEYS:
            assert np.array_equal(r[k], res[0][k]), k
    r0 = res[0]
    assert r0["exchange"] == 3.0
    assert int(r0["trial_launches"]) == 10 and int(r0["check_launches"]) == 27  # (folded ranks: single-block waits, fusedWait 0)
    assert int(r0["term"]) == 0 and int(r0["num_restarts"]) > 0
    lp = _qp(name)
    ref = REF_SPARSE[name]["objective_value"]
    obj = lp.objective_value(r0["col_value"])
    assert abs(obj - ref) <= 1e-6 * (1 + abs(ref)), (obj, ref)


@pytest.mark.parametrize("exchange", ["mesh", "rccl"])
def test_sharded_sequence_on_one_rank_reaches_the_single_gpu_optimum(exchange, monkeypatch):
    """PDLP_MI355X_FORCE_COMM=1: the sharded kernel sequence of either exchange on a single rank."""
    name = "sq102"
    lp = _qp(name)
    kw = dict(kkt_tolerance=1e-8, pdlp_iteration_limit=400000)
    base = solver.solveLpCupdlp(lp, **kw)
    assert base.model_status == solver.kOptimal
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    monkeypatch.setenv("PDLP_MI355X_EXCHANGE", exchange)
    sh = solver.solveLpCupdlp(lp, time_limit=1000.0, **kw)
    assert sh.model_status == solver.kOptimal, solver.lib().pdlp_mi355x_last_error()
    a, b = sh.info["objective_function_value"], base.info["objective_function_value"]
    assert abs(a - b) <= 1e-6 * (1 + abs(b))
    ref = REF_SPARSE[name]["objective_value"]
    assert abs(a - ref) <= 1e-6 * (1 + abs(ref))
    assert 0.5 * base.pdlp_iteration_count <= sh.pdlp_iteration_count <= 2 * base.pdlp_iteration_count
    S = solver.DeviceSolver(lp=lp)
    try:
        assert S.stage("exchange")[0] == (3.0 if exchange == "mesh" else 1.0)
        # LP + 1: RCCL 7 + 1; the mesh 5 + 1 with one launch per exchange (a rank with a GPU of its own), else 9 + 1
        assert S.stage("trial_launches")[0] in ((6.0, 10.0) if exchange == "mesh" else (8.0,))
    finally:
        S.close()


@pytest.mark.parametrize("slab", ["0", "1"])
@pytest.mark.parametrize("name,k", [("sq102", 60), ("band40k", 60)])
@pytest.mark.parametrize("world", [2, 4])
def test_fixed_iterations_match_single_gpu(world, name, k, slab, tmp_path, monkeypatch):
    """K trials over rank processes against DeviceSolver.iterate(K) on one GPU, with the row slice of N in the CSR-stream
    and in the slab layout (PDLP_MI355X_SLAB; the automatic choice takes the slab layout only from a 2 MB gathered vector).
    The ranks hold the same bits; against one GPU only the grouping of the reduction partials differs."""
    sys.path.insert(0, HERE)
    from qp_mesh_worker import qp_problem
    monkeypatch.setenv("PDLP_MI355X_SLAB", slab)
    S = solver.DeviceSolver(lp=qp_problem(name))
    try:
        S.iterate(k)
        x1 = S.get("x", S.n)
    finally:
        S.close()
    res = _run_ranks(world, f"iterate:{name}:{k}", tmp_path, extra_env={"PDLP_MI355X_SLAB": slab})
    for r in res[1:]:
        assert np.array_equal(r["x"], res[0]["x"]) and np.array_equal(r["steps"], res[0]["steps"])
    assert int(res[0]["iters"]) == k
    assert int(res[0]["trial_launches"]) == 10  # 9 of an LP (fusedWait 0) + N x+
    err = np.linalg.norm(res[0]["x"] - x1) / (1e-300 + np.linalg.norm(x1))
    assert err < 1e-9, err


def test_device_and_host_driven_checks_give_the_same_bits(tmp_path):
    """The sharded check on the device (N xAvg after the all-gather of xAvg, its 1/2 x'Qx in the statistics' all-reduce, nx
    restarted to N xAvg) and driven from the host (PDLP_MI355X_DEVICE_CHECK=0): whole solves, the same bits."""
    a = _run_ranks(2, "solve:sq100", tmp_path / "dev")
    b = _run_ranks(2, "solve:sq100", tmp_path / "host", extra_env={"PDLP_MI355X_DEVICE_CHECK": "0"})
    assert int(b[0]["check_launches"]) == 0
    for r in range(2):
        for k in _SOLVE_KEYS:
            assert np.array_equal(a[r][k], b[r][k]), (r, k)
            assert np.array_equal(a[0][k], a[r][k]), (r, k)
    assert int(a[0]["num_restarts"]) > 0 and int(a[0]["term"]) == 0


def test_exchange_forms_give_the_same_bits(tmp_path):
    """PDLP_MI355X_MESH_FUSED_WAIT 0 (single-block waits), 1 (consumers that wait themselves) and 2 (an exchange per launch,
    the form of ranks on GPUs of their own): 10, 8 and 6 launches per trial, 27, 27 and 15 per check, the same solve bit
    for bit."""
    a = _run_ranks(2, "solve:sq100", tmp_path / "w0", extra_env={"PDLP_MI355X_MESH_FUSED_WAIT": "0"})
    assert (int(a[0]["trial_launches"]), int(a[0]["check_launches"])) == (10, 27)
    for level, launches in (("1", (8, 27)), ("2", (6, 15))):
        b = _run_ranks(2, "solve:sq100", tmp_path / ("w" + level), extra_env={"PDLP_MI355X_MESH_FUSED_WAIT": level})
        assert (int(b[0]["trial_launches"]), int(b[0]["check_launches"])) == launches, level
        for r in range(2):
            for k in _SOLVE_KEYS:
                assert np.array_equal(a[r][k], b[r][k]), (level, r, k)
                assert np.array_equal(b[0][k], b[r][k]), (level, r, k)
