"""pdlp_mi355x_update on the device: a held solver, updated in place, must be in the state of a fresh
pdlp_mi355x_create on the modified problem — the same bits in the device's cost / rhs / bounds right after the update,
in every solution vector, count and residual after a run, and in the iterates after a fixed number of iterations — in
every loop form (persistent small-LP loop, 3-launch stream form, fused slab form with and without task workgroups, QPs
with a diagonal and a sparse Hessian), from both set-up paths.  The oracle is code that exists without this feature:
create() on P' built in Python."""
import os

import numpy as np
import pytest

import lpgen
import update_cases as UC
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=20000)
DATA = ("cost", "rhs", "lower", "upper")
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")


def _ctest(name):
    return L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz"))


def _synthetic(m, n, nnz):
    sp = solver.SyntheticProblem(m, n, nnz, 1)
    lp = sp.to_lp()
    sp.close()
    return lp


MAKERS = {
    "adlittle": lambda: _ctest("adlittle"),             # persistent loop, one-launch check
    "25fv47": lambda: _ctest("25fv47"),
    "scrs8": lambda: _ctest("scrs8"),
    "random_lp": lambda: lpgen.random_lp(5),            # ranged and free rows: slack bounds move
    "synthetic_100k": lambda: _synthetic(100_000, 100_000, 1_000_000),  # persistent, hierarchical barrier, device set-up
    "structured_lp": lambda: lpgen.structured_lp(),     # fused slab form
    "dense_column_lp": lambda: lpgen.dense_column_lp(),  # slab form with task workgroups
    "tall_lp": lambda: lpgen.tall_lp(),
    "random_diag_qp": lambda: lpgen.random_diag_qp(3),
    "random_sparse_qp": lambda: lpgen.random_sparse_qp(3),
}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name]()
    return _cache[name]


def _create(lp, start=None, **options):
    """DeviceSolver on lp (with a hot start in the problem struct when `start` is given)."""
    if start is None:
        return solver.DeviceSolver(lp, **dict(OPTIONS, **options))
    handle = abi.ProblemHandle(lp, start)
    ds = solver.DeviceSolver(problem_struct=handle.struct, **dict(OPTIONS, **options))
    ds._keep = handle
    return ds


def _data(ds):
    return {k: ds.get(k, ds.m if k == "rhs" else ds.n) for k in DATA}


def _assert_same_data(a, b):
    da, db = _data(a), _data(b)
    for k in DATA:
        assert np.array_equal(da[k], db[k]), k


def _assert_same_result(a, b):
    for k in SOLUTION:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in COUNTS:
        assert getattr(a, k) == getattr(b, k), k
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))


def _everything(lp):
    """The update that brings a solver to lp's data whatever it held before."""
    return dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)


def _check_updates(name, kinds=UC.KINDS, **options):
    """One held solver; every modification is applied to the ORIGINAL data (each array alone reaches the device as the
    only one given), compared with a fresh solver on P', and taken back."""
    lp = _lp(name)
    held = _create(lp, updatable=True, **options)
    for what in kinds:
        u = UC.modification(lp, what, seed=len(name) + 7)
        lp2 = UC.apply(lp, u)
        held.update(**u)
        fresh = _create(lp2, **options)
        _assert_same_data(held, fresh)
        _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
        fresh.close()
        held.update(**_everything(lp))
    fresh = _create(lp, **options)
    _assert_same_data(held, fresh)
    fresh.close()
    held.close()


# ---- 5: every loop form, every kind of modification, both set-up paths ---------------------------------------------
@pytest.mark.parametrize("gpu_setup", ["0", "1"])
@pytest.mark.parametrize("name", ["adlittle", "25fv47", "scrs8", "random_lp", "random_diag_qp", "synthetic_100k"])
def test_update_equals_fresh_create_from_both_setups(name, gpu_setup, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", gpu_setup)
    _check_updates(name)


@pytest.mark.parametrize("name", ["structured_lp", "dense_column_lp", "tall_lp", "random_sparse_qp"])
def test_update_equals_fresh_create(name):
    _check_updates(name)


def test_update_equals_fresh_create_maximise_and_without_scaling():
    import copy
    lp = copy.copy(_lp("25fv47"))
    lp.sense = -1
    _cache["25fv47_max"] = lp
    _check_updates("25fv47_max", kinds=("all",))
    _check_updates("scrs8", kinds=("all",), pdlp_features_off=abi.FEATURE_SCALING_OFF)


# ---- 6: a chain on one solver ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["25fv47", "structured_lp", "random_sparse_qp"])
def test_chain_of_updates_on_one_solver(name):
    lp = _lp(name)
    lp_a = UC.apply(lp, UC.modification(lp, "all", seed=21))
    lp_b = UC.apply(lp, UC.modification(lp, "row_bounds", seed=22))
    held = _create(lp, updatable=True)
    results = [held.run(lp.num_col, lp.num_row)]
    for target in (lp_a, lp_b, lp):
        held.update(**_everything(target))
        results.append(held.run(lp.num_col, lp.num_row))
    held.close()
    for target, got in zip((lp, lp_a, lp_b, lp), results):
        fresh = _create(target)
        _assert_same_result(got, fresh.run(lp.num_col, lp.num_row))
        fresh.close()
    _assert_same_result(results[0], results[3])


# ---- 7: the bench LP, fused slab form: per-block bounds and the captured graph follow the update -----------------
def _iterate_state(ds, iters=200):
    st = ds.iterate(iters)
    out = {k: ds.get(k, ds.m if k in ("y", "ax") else ds.n) for k in ("x", "y", "ax", "aty")}
    out["counts"] = (st.iters, st.trials, st.restarts)
    return out


def _assert_same_state(a, b):
    assert a["counts"] == b["counts"]
    for k in ("x", "y", "ax", "aty"):
        assert np.array_equal(a[k], b[k]), k


def test_update_at_bench_size_flips_lower_uniform_both_ways(monkeypatch):
    lp = _synthetic(1_000_000, 1_000_000, 8_000_000)
    opts = dict(kkt_tolerance=1e-4)
    held = solver.DeviceSolver(lp, updatable=True, **opts)
    assert held.stage("trial_launches")[0] == 2.0          # the fused form
    assert held.stage("update_state")[2] == 1.0            # box 0 <= x <= 1: one lower bound for all columns
    # A: new costs and row bounds, and ONE column with lower bound 0.5 — the ULO instantiation no longer applies
    u = UC.modification(lp, "cost", seed=31)
    u["row_lower"], u["row_upper"] = UC.new_row_bounds(lp, np.random.default_rng(32))
    lo = np.array(lp.col_lower)
    lo[lp.num_col // 3] = 0.5
    u["col_lower"] = lo
    lp_a = UC.apply(lp, u)
    held.update(**u)
    assert held.stage("update_state")[2] == 0.0
    got_a = _iterate_state(held)
    fresh = solver.DeviceSolver(lp_a, **opts)
    assert fresh.stage("update_state")[2] == 0.0
    _assert_same_data(held, fresh)
    want_a = _iterate_state(fresh)
    fresh.close()
    _assert_same_state(got_a, want_a)
    # ... and the 3-launch form computes the same bits as the fused one after the update
    monkeypatch.setenv("PDLP_MI355X_FUSED", "0")
    plain = solver.DeviceSolver(lp_a, **opts)
    assert plain.stage("trial_launches")[0] == 3.0
    _assert_same_state(got_a, _iterate_state(plain))
    plain.close()
    monkeypatch.delenv("PDLP_MI355X_FUSED")
    # B: back to the original data — one lower bound for all columns again
    held.update(**_everything(lp))
    assert held.stage("update_state")[2] == 1.0
    got_b = _iterate_state(held)
    fresh = solver.DeviceSolver(lp, **opts)
    _assert_same_data(held, fresh)
    want_b = _iterate_state(fresh)
    fresh.close()
    held.close()
    _assert_same_state(got_b, want_b)


# ---- 8: hot start -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e226", "structured_lp"])
def test_update_with_hot_start_equals_fresh_create_with_start(name):
    lp = _ctest(name) if name == "e226" else _lp(name)
    held = _create(lp, updatable=True)
    first = held.run(lp.num_col, lp.num_row)
    start = dict(col_value=first.col_value.copy(), row_value=first.row_value.copy(), row_dual=first.row_dual.copy())
    u = UC.modification(lp, "cost", seed=41)
    lp2 = UC.apply(lp, u)
    held.update(start=start, **u)
    got = held.run(lp.num_col, lp.num_row)
    fresh = _create(lp2, start=start)
    want = fresh.run(lp.num_col, lp.num_row)
    fresh.close()
    _assert_same_result(got, want)
    # the start is not sticky: the next update without one is a cold start
    held.update()
    cold = _create(lp2)
    _assert_same_result(held.run(lp.num_col, lp.num_row), cold.run(lp.num_col, lp.num_row))
    cold.close()
    held.close()


# ---- 9: refusals with a handle leave the solver as it was ---------------------------------------------------------
def _refused(ds, **u):
    with pytest.raises(RuntimeError) as e:
        ds.update(**u)
    return str(e.value)


def test_refused_without_updatable():
    lp = _lp("adlittle")
    ds, untouched = _create(lp), _create(lp)
    assert ds.stage("update_state")[0] == 0.0  # nothing kept
    assert "updatable" in _refused(ds, col_cost=lp.col_cost * 2.0)
    _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
    ds.close(); untouched.close()


def test_refused_for_hipdlp():
    lp = _lp("adlittle")
    ds, untouched = _create(lp, solver="hipdlp", updatable=True), _create(lp, solver="hipdlp")
    assert "HiPDLP" in _refused(ds, col_cost=lp.col_cost * 2.0)
    a, b = ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row)
    for k in SOLUTION:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.num_iter == b.num_iter and a.term_code == b.term_code
    ds.close(); untouched.close()


def test_refused_for_a_sharded_solver(monkeypatch):
    lp = _lp("adlittle")
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    ds, untouched = _create(lp, updatable=True), _create(lp)
    assert "sharded" in _refused(ds, col_cost=lp.col_cost * 2.0)
    _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
    ds.close(); untouched.close()


@pytest.mark.parametrize("name", ["25fv47", "structured_lp"])
def test_refused_row_kind_change_changes_nothing(name):
    lp = _lp(name)
    ds, untouched = _create(lp, updatable=True), _create(lp)
    kind = UC.row_kind(np.asarray(lp.row_lower), np.asarray(lp.row_upper))
    eq = np.nonzero(kind == 0)[0]
    lo, up = np.array(lp.row_lower), np.array(lp.row_upper)
    rows = sorted(int(i) for i in (eq[eq.size // 3], eq[-1]))
    for i in rows:
        up[i] = lo[i] + 1.0  # equality -> ranged
    before = _data(ds)
    msg = _refused(ds, col_cost=lp.col_cost * 2.0, col_lower=lp.col_lower - 1.0, row_lower=lo, row_upper=up, offset=9.0)
    assert f"row {rows[0]} " in msg and "equality" in msg and "ranged or free" in msg
    after = _data(ds)
    for k in DATA:
        assert np.array_equal(before[k], after[k]), k
    _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
    # a partial start and a lone row bound are refused the same way
    assert "partial start" in _refused(ds, start=dict(col_value=np.zeros(lp.num_col)))
    assert "row_upper is NULL" in _refused(ds, row_lower=lo)
    _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
    ds.close(); untouched.close()


# ---- 10: the flag alone changes nothing --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["25fv47", "synthetic_100k", "structured_lp"])
def test_updatable_solver_never_updated_equals_default(name):
    lp = _lp(name)
    a, b = _create(lp, updatable=True), _create(lp)
    assert a.stage("update_state")[0] > 0.0 and b.stage("update_state")[0] == 0.0
    _assert_same_data(a, b)
    _assert_same_result(a.run(lp.num_col, lp.num_row), b.run(lp.num_col, lp.num_row))
    a.close(); b.close()


def test_solve_returns_what_solveLpCupdlp_returns():
    """create once; for each: update, solve."""
    lp = _lp("25fv47")
    held = solver.DeviceSolver(lp, updatable=True, **OPTIONS)
    for seed in (51, 52):
        u = UC.modification(lp, "all", seed=seed)
        held.update(**u)
        got = held.solve()
        want = solver.solveLpCupdlp(UC.apply(lp, u), **OPTIONS)
        assert got.model_status == want.model_status and got.pdlp_iteration_count == want.pdlp_iteration_count
        for k in SOLUTION:
            assert np.array_equal(getattr(got.solution, k), getattr(want.solution, k)), k
        assert got.info["objective_function_value"] == want.info["objective_function_value"]
        assert got.result.setup_seconds > 0.0  # the time the update took
    held.close()
