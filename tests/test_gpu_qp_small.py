"""Small QPs with off-diagonal Hessian entries in the persistent trial loop (pdlp_small.hip QOFF) and the one-launch check
(pdlp_check.hip): whole solves bit for bit against the oracle's device-order mode, the switch PDLP_MI355X_PERSISTENT_QP
on / off, hot starts, value updates, batches (eight variants at once, one per XCD) and pools (such a QP runs alone).
No tolerance anywhere: every comparison is `==` / array_equal.

Shapes, each chosen for what only it can break:
  sq0           20 columns: ONE workgroup holds every block of A, A' and N — the body without cross-workgroup traffic
  sq100         200 x 61, A in 9 blocks, N in 3: XCD-local mode; workgroups 3..8 have no block of N
  portfolio64   dense Q on 64 columns, two rows: N in 8 blocks, A and A' in one — the grid is set by N, and workgroups
                without a block of A or A' still step columns and meet the barriers
  sq101         500 x 161, A in 69 blocks: more than 32 workgroups — agent-scope accesses on all XCDs, hierarchical barrier;
                more than 64: the check stays ten launches behind the persistent loop
  dense600      dense Q on 600 columns (rows of N have 599 entries): does NOT qualify, says why, still bit-equal
  arrow700      one row of N with 699 entries among 512-entry blocks (a long major): does not qualify either
Coverage of the capped runs, checked with the oracle alone when the caps were picked (and asserted below):
  a rejected trial (num_trials > num_iter; nx of the next parity is overwritten without a parity swap): sq100 (209 trials
  for 200 iterations), portfolio64 (338 / 320), sq101 (290 / 280); sq0 accepts all of its 360
  a restart (nx <- N xAvg inside the check): every case (nine restarts each)"""
import os

import numpy as np
import pytest

import oraclelib as O
import qp_small_cases as QC
import update_cases as UC
import update_hessian_cases as HC
import update_matrix_cases as MC
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "term_iterate", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")


def _golden(name):
    return lambda: L.HighsLp.from_npz(os.path.join(GOLD, "qp" if name.startswith(("sq", "qp")) else "instances", name + ".npz"))


# name -> (maker, iteration cap of the whole-solve comparison)
CASES = {
    "sq0": (_golden("sq0"), 4000),
    "sq100": (_golden("sq100"), 4000),
    "portfolio64": (QC.portfolio, 4000),
    "sq101": (_golden("sq101"), 4000),
    "dense600": (QC.dense_hessian, 400),
    "arrow700": (QC.arrow_hessian, 400),
}
QUALIFYING = ("sq0", "sq100", "portfolio64", "sq101")
WITH_REJECTION = ("sq100", "portfolio64", "sq101")
_lps, _oracles = {}, {}


def _lp(name):
    if name not in _lps:
        _lps[name] = _golden(name)() if name not in CASES else CASES[name][0]()
    return _lps[name]


def _kw(name):
    return dict(kkt_tolerance=1e-7, pdlp_iteration_limit=CASES[name][1])


def _oracle(name, start=None, tag=None):
    """The oracle's solve in the device's reduction order (computed once per case and start, shared, never changed)."""
    if (name, tag) not in _oracles:
        _oracles[(name, tag)] = O.oracle_solve(_lp(name), start=start, device_reduction_order=True, device_layout="csr", **_kw(name))
    return _oracles[(name, tag)]


def _assert_equals_oracle(gpu, cpu):
    R = gpu.result
    assert (R.term_code, R.num_iter, R.num_trials, R.num_restarts) == (cpu.term_code, cpu.num_iter, cpu.num_trials, cpu.num_restarts)
    assert R.primal_obj == cpu.primal_obj and R.dual_obj == cpu.dual_obj
    assert np.array_equal(gpu.solution.col_value, cpu.col_value) and np.array_equal(gpu.solution.row_dual, cpu.row_dual)
    assert np.array_equal(gpu.solution.col_dual, cpu.col_dual)


def _assert_same_result(got, want, what=""):
    for k in SOLUTION:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
    for k in COUNTS + SCALARS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


# ---- 1, 2: whole solves against the oracle -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", QUALIFYING)
def test_whole_solve_is_one_persistent_loop_with_the_oracles_bits(name, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    lp = _lp(name)
    cpu = _oracle(name)
    print(name, "oracle: iterations", cpu.num_iter, "trials", cpu.num_trials, "restarts", cpu.num_restarts)
    if name in WITH_REJECTION:
        assert cpu.num_trials > cpu.num_iter  # a rejected trial inside the capped run
    assert cpu.num_restarts >= 1  # nx <- N xAvg is taken
    ds = solver.DeviceSolver(lp, **_kw(name))
    barriers, checks = ds.stage("trial_barriers", 1)[0], ds.stage("check_launches", 1)[0]
    gpu = ds.solve()
    launches = ds.stage("persistent_launches", 1)[0]
    ds.close()
    print(name, "trial_barriers", barriers, "check_launches", checks, "persistent_launches", launches)
    assert barriers == 3 and launches > 0
    P = solver.Prepared(lp)  # the grid: the most work blocks of an operand (N's exceed A's in portfolio64 only: 8)
    grid = max(P.spmv_blocks_ax, P.spmv_blocks_aty, 8 if name == "portfolio64" else 0)
    assert (grid > 64) == (name == "sq101")  # (sq101: 69 blocks of A)
    assert checks == (1 if grid <= 64 else 10)  # the one-launch check takes at most 64 workgroups
    _assert_equals_oracle(gpu, cpu)


@pytest.mark.parametrize("name,words", [("dense600", "N streams in 2048-entry blocks"), ("arrow700", "N has a long major")])
def test_a_qp_that_does_not_qualify_keeps_its_launches_and_says_why(name, words, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    lp = _lp(name)
    ds = solver.DeviceSolver(lp, **_kw(name))
    assert ds.stage("trial_barriers", 1)[0] == 0 and ds.stage("check_launches", 1)[0] == 10
    gpu = ds.solve()
    assert ds.stage("persistent_launches", 1)[0] == 0
    ds.close()
    _assert_equals_oracle(gpu, _oracle(name))
    batch = solver.DeviceBatch(lp, lanes=2, **_kw(name))
    batch.run([{}])
    I = batch.info()
    batch.close()
    assert I.lanes_concurrent == 1 and I.text.startswith("sequential: ") and words in I.text, I.text


# ---- 3: the switch -----------------------------------------------------------------------------------------------------------
def _state(ds):
    out = {k: ds.get(k, ds.m if k == "y" else ds.n) for k in ("x", "y", "nx", "aty")}
    out["steps"] = ds.get("steps", 8)
    return out


@pytest.mark.parametrize("name,local", [("sq100", "1"), ("portfolio64", "1"), ("sq100", "0")])
def test_switch_off_gives_the_same_iterates_and_the_same_solve(name, local, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    if local == "0":
        monkeypatch.setenv("PDLP_MI355X_XCD_LOCAL", "0")
    lp = _lp(name)
    on = solver.DeviceSolver(lp, **_kw(name))
    monkeypatch.setenv("PDLP_MI355X_PERSISTENT_QP", "0")  # (switches are read at create)
    off = solver.DeviceSolver(lp, **_kw(name))
    monkeypatch.delenv("PDLP_MI355X_PERSISTENT_QP")
    assert on.stage("trial_barriers", 1)[0] == 3 and off.stage("trial_barriers", 1)[0] == 0
    assert off.stage("trial_launches", 1)[0] == 3 and off.stage("check_launches", 1)[0] == 10
    for iters in (40, 1):  # after 40 and after 41 iterations: both parities of the buffers
        a, b = on.iterate(iters), off.iterate(iters)
        assert (a.iters, a.trials, a.restarts) == (b.iters, b.trials, b.restarts)
        sa, sb = _state(on), _state(off)
        for k in sa:
            assert np.array_equal(sa[k], sb[k]), (iters, k)
    assert np.any(_state(on)["nx"] != 0.0)
    on.reset(); off.reset()
    _assert_same_result(on.run(lp.num_col, lp.num_row), off.run(lp.num_col, lp.num_row), name)
    assert on.stage("persistent_launches", 1)[0] > 0 and off.stage("persistent_launches", 1)[0] == 0
    assert on.stage("barrier_fallbacks", 1)[0] == 0
    on.close(); off.close()


# ---- 4: hot start ------------------------------------------------------------------------------------------------------------
def test_hot_start_has_the_oracles_bits(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    name = "sq100"
    lp = _lp(name)
    first = O.oracle_solve(lp, device_reduction_order=True, device_layout="csr", **dict(_kw(name), pdlp_iteration_limit=80))
    assert first.num_iter == 79  # (stopped at its limit: a start that is on the way, not the solution)
    start = dict(col_value=np.array(first.col_value), row_value=lp.row_activity(first.col_value), row_dual=np.array(first.row_dual))
    cpu = _oracle(name, start=start, tag="hot")
    cold = _oracle(name)
    assert cpu.num_iter > 40 and (cpu.num_iter, cpu.num_trials) != (cold.num_iter, cold.num_trials)  # (the start changed the run)
    gpu = solver.solveLpCupdlp(lp, start=start, **_kw(name))
    _assert_equals_oracle(gpu, cpu)


# ---- 5: updates --------------------------------------------------------------------------------------------------------------
def test_value_updates_stay_on_the_persistent_path_and_equal_a_fresh_create(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    name = "sq100"
    lp = _lp(name)
    options = dict(_kw(name), updatable="matrix+hessian")
    held = solver.DeviceSolver(lp, **options)
    assert held.stage("trial_barriers", 1)[0] == 3
    target = lp
    for u in (HC.modification(lp, "regen", seed=41), MC.modification(lp, "all", seed=43)):
        held.update_values(**u)
        target = HC.apply(target, u)
        assert held.stage("trial_barriers", 1)[0] == 3 and held.stage("check_launches", 1)[0] == 1
        before = held.stage("persistent_launches", 1)[0]
        got = held.run(lp.num_col, lp.num_row)
        assert held.stage("persistent_launches", 1)[0] > before
        fresh = solver.DeviceSolver(target, **options)
        _assert_same_result(got, fresh.run(lp.num_col, lp.num_row), sorted(u))
        fresh.close()
    held.close()


# ---- 6: batches --------------------------------------------------------------------------------------------------------------
BATCH = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)
_solo = {}


def _everything(lp):
    return dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)


def _solo_variant(name, tag, u):
    """(result, persistent launches) of update(u) + run on one held solver of its own (computed once per variant)."""
    if (name, tag) not in _solo:
        lp = _lp(name)
        held = solver.DeviceSolver(lp, updatable=True, **BATCH)
        held.update(**dict(_everything(lp), **u))
        before = held.stage("persistent_launches", 1)[0]
        R = held.run(lp.num_col, lp.num_row)
        _solo[(name, tag)] = (R, int(held.stage("persistent_launches", 1)[0] - before))
        held.close()
    return _solo[(name, tag)]


@pytest.mark.parametrize("K", [8, 11])
def test_batch_runs_eight_variants_at_once(K):
    name = "sq100"
    lp = _lp(name)
    kinds = (["cost", "col_bounds", "row_bounds"] * 4)[:K]
    tagged = [(what + str(3 + i), UC.modification(lp, what, 3 + i)) for i, what in enumerate(kinds)]
    refs = [_solo_variant(name, tag, u) for tag, u in tagged]
    batch = solver.DeviceBatch(lp, lanes=8, **BATCH)
    out = batch.run([u for _, u in tagged])
    I = batch.info()
    batch.close()
    print("batch info:", I.text, I.lanes_concurrent, I.trial_launches, I.check_launches, [r[1] for r in refs])
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (8, 8, K, 0), I.text
    for (tag, _), o, ref in zip(tagged, out, refs):
        _assert_same_result(o.result, ref[0], tag)
    if K == 8:  # (nothing is refilled: the bound of tests/test_gpu_batch.py)
        assert I.trial_launches <= max(r[1] for r in refs) + 15, (I.trial_launches, [r[1] for r in refs])
        assert I.check_launches == I.trial_launches + 1


# ---- 7: pools ----------------------------------------------------------------------------------------------------------------
def test_pool_runs_such_qps_alone_and_the_lps_shared():
    names = ["sq100", "25fv47", "sq0", "adlittle"]
    lps = [_lp(n) for n in names]
    solos = [solver.solveLpCupdlp(lp, **BATCH).result for lp in lps]
    out, I = solver.solve_many(lps, lanes=4, **BATCH)
    paths = [o.info["pool_path"] for o in out]
    print("pool:", paths, I.text)
    assert paths == [abi.POOL_ALONE, abi.POOL_SHARED, abi.POOL_ALONE, abi.POOL_SHARED], (paths, I.text)
    assert "off-diagonal Hessian: not in shared pool launches" in I.text, I.text
    for n, o, ref in zip(names, out, solos):
        _assert_same_result(o.result, ref, n)
