"""pdlp_mi355x_update_matrix on the device: a held solver whose matrix VALUES are replaced in place (same sparsity
pattern) must be in the state of a fresh pdlp_mi355x_create on the modified problem — the same bits in the device's cost
/ rhs / bounds / scale vectors right after the update, in A x and A' y on fixed random vectors, in every solution
vector, count and residual after a run, and in the iterates after a fixed number of iterations — in every loop form and
from both set-up paths.  The oracle is code that exists without this feature: create() on P' built in Python
(tests/update_matrix_cases.py).  No tolerance anywhere."""
import os

import numpy as np
import pytest

import lpgen
import update_cases as UC
import update_matrix_cases as MC
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=20000)
DATA = ("cost", "rhs", "lower", "upper", "col_scale", "row_scale")
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
    "random_lp": lambda: lpgen.random_lp(5),            # ranged and free rows: slack entries, slack bounds
    "synthetic_100k": lambda: _synthetic(100_000, 100_000, 1_000_000),  # persistent, hierarchical barrier, device set-up
    "structured_lp": lambda: lpgen.structured_lp(),     # fused slab form
    "dense_column_lp": lambda: lpgen.dense_column_lp(),  # slab form with task workgroups
    "tall_lp": lambda: lpgen.tall_lp(),                 # long majors
    "random_diag_qp": lambda: lpgen.random_diag_qp(3),
    "random_sparse_qp": lambda: lpgen.random_sparse_qp(3),
}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name]()
    return _cache[name]


def _create(lp, start=None, **options):
    if start is None:
        return solver.DeviceSolver(lp, **dict(OPTIONS, **options))
    handle = abi.ProblemHandle(lp, start)
    ds = solver.DeviceSolver(problem_struct=handle.struct, **dict(OPTIONS, **options))
    ds._keep = handle
    return ds


def _data(ds):
    return {k: ds.get(k, ds.m if k in ("rhs", "row_scale") else ds.n) for k in DATA}


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


def _products(ds, seed=77):
    """A x and A' y of the solver's operands — every value array the loops read — on fixed random vectors."""
    rng = np.random.default_rng(seed)
    x, y = rng.standard_normal(ds.n), rng.standard_normal(ds.m)
    ds.set("x", x); ds.stage("ax")
    ds.set("y", y); ds.stage("aty")
    return ds.get("ax", ds.m), ds.get("aty", ds.n)


def _assert_same_products(a, b):
    (ax_a, aty_a), (ax_b, aty_b) = _products(a), _products(b)
    assert np.array_equal(ax_a, ax_b), "ax"
    assert np.array_equal(aty_a, aty_b), "aty"


def _everything(lp):
    return dict(a_value=lp.a_value, col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper,
                row_lower=lp.row_lower, row_upper=lp.row_upper, offset=lp.offset)


def _has_zero_inside_a_long_major(lp, a, limit=256):
    start = np.asarray(lp.a_start, dtype=np.int64)
    rows = np.asarray(lp.a_index, dtype=np.int64)
    cols = np.repeat(np.arange(lp.num_col), np.diff(start))
    zero = a == 0.0
    long_cols = np.diff(start) > limit
    long_rows = np.bincount(rows, minlength=lp.num_row) > limit
    return bool(np.any(zero & long_cols[cols]) or np.any(zero & long_rows[rows]))


def _check_matrix_updates(name, kinds=("values", "all"), need_long_zero=False, **options):
    """One held solver; every modification is applied to the ORIGINAL problem, compared with a fresh solver on P' (data,
    a run, then the products: the run starts from the update's own reset), and finally taken back."""
    lp = _lp(name)
    held = _create(lp, updatable="matrix", **options)
    assert held.stage("update_state")[5] == 1.0 and held.stage("update_state")[4] > 0.0
    for what in kinds:
        u = MC.modification(lp, what, seed=len(name) + 13)
        if need_long_zero:
            assert _has_zero_inside_a_long_major(lp, u["a_value"]), "the case must zero an entry of a long major"
        lp2 = MC.apply(lp, u)
        held.update_matrix(**u)
        fresh = _create(lp2, **options)
        _assert_same_data(held, fresh)
        _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
        _assert_same_products(held, fresh)
        fresh.close()
    held.update_matrix(**_everything(lp))
    fresh = _create(lp, **options)
    _assert_same_data(held, fresh)
    _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
    _assert_same_products(held, fresh)
    fresh.close()
    held.close()


# ---- every loop form, both set-up paths ------------------------------------------------------------------------------
@pytest.mark.parametrize("gpu_setup", ["0", "1"])
@pytest.mark.parametrize("name", ["adlittle", "25fv47", "scrs8", "random_lp", "random_diag_qp", "synthetic_100k"])
def test_update_matrix_equals_fresh_create_from_both_setups(name, gpu_setup, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", gpu_setup)
    _check_matrix_updates(name)


@pytest.mark.parametrize("name", ["structured_lp", "dense_column_lp", "tall_lp"])
def test_update_matrix_equals_fresh_create(name):
    """The fused slab form, task workgroups and long majors; the zeroed entries include one inside a long major."""
    _check_matrix_updates(name, need_long_zero=True)


def test_update_matrix_equals_fresh_create_maximise_and_without_scaling():
    import copy
    lp = copy.copy(_lp("25fv47"))
    lp.sense = -1
    _cache["25fv47_max"] = lp
    _check_matrix_updates("25fv47_max", kinds=("all",))
    _check_matrix_updates("scrs8", kinds=("all",), pdlp_features_off=abi.FEATURE_SCALING_OFF)


def test_update_matrix_without_scaling_from_the_device_setup(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", "1")
    _check_matrix_updates("scrs8", kinds=("all",), pdlp_features_off=abi.FEATURE_SCALING_OFF)
    _check_matrix_updates("synthetic_100k", kinds=("all",), pdlp_features_off=abi.FEATURE_SCALING_OFF)


# ---- a chain on one solver: update_matrix -> update (costs only) -> update_matrix back ------------------------------------
@pytest.mark.parametrize("name", ["25fv47", "structured_lp"])
def test_chain_of_matrix_and_data_updates_on_one_solver(name):
    lp = _lp(name)
    u_a = MC.modification(lp, "values", seed=21)
    lp_a = MC.apply(lp, u_a)
    u_b = UC.modification(lp_a, "cost", seed=22)   # replays the factors of lp_a's matrix
    lp_b = UC.apply(lp_a, u_b)
    held = _create(lp, updatable="matrix")
    results = [held.run(lp.num_col, lp.num_row)]
    held.update_matrix(**u_a)
    results.append(held.run(lp.num_col, lp.num_row))
    held.update(**u_b)
    results.append(held.run(lp.num_col, lp.num_row))
    held.update_matrix(**_everything(lp))
    results.append(held.run(lp.num_col, lp.num_row))
    for target, got in zip((lp, lp_a, lp_b, lp), results):
        fresh = _create(target)
        _assert_same_result(got, fresh.run(lp.num_col, lp.num_row))
        if target is lp and got is results[3]:
            _assert_same_data(held, fresh)
            _assert_same_products(held, fresh)
        fresh.close()
    held.close()
    _assert_same_result(results[0], results[3])


# ---- the bench LP: fused slab form at 1M x 1M ----------------------------------------------------------------------
def _iterate_state(ds, iters=200):
    st = ds.iterate(iters)
    out = {k: ds.get(k, ds.m if k in ("y", "ax") else ds.n) for k in ("x", "y", "ax", "aty")}
    out["counts"] = (st.iters, st.trials, st.restarts)
    return out


def _assert_same_state(a, b):
    assert a["counts"] == b["counts"]
    for k in ("x", "y", "ax", "aty"):
        assert np.array_equal(a[k], b[k]), k


def test_update_matrix_at_bench_size():
    lp = _synthetic(1_000_000, 1_000_000, 8_000_000)
    opts = dict(kkt_tolerance=1e-4)
    held = solver.DeviceSolver(lp, updatable="matrix", **opts)
    assert held.stage("trial_launches")[0] == 2.0          # the fused form
    u = MC.modification(lp, "all", seed=31)
    held.update_matrix(**u)
    kept = held.stage("update_state")
    secs = held.stage("update_matrix_seconds")
    print("1M x 1M: update_matrix %.2f ms (upload+validation %.2f, formulate %.2f, passes %.2f, refills %.2f, norms+sums %.2f, "
          "block bounds %.2f, graph %.2f, reset %.2f); kept %.1f MB + %.1f MB = %.1f B per nonzero" %
          (1e3 * secs[8], *(1e3 * secs[:8]), kept[0] / 1e6, kept[4] / 1e6, kept[4] / held.nnz))
    got = _iterate_state(held)
    held_data = _data(held)
    held.close()
    fresh = solver.DeviceSolver(MC.apply(lp, u), **opts)
    fresh_data = _data(fresh)
    for k in DATA:
        assert np.array_equal(held_data[k], fresh_data[k]), k
    want = _iterate_state(fresh)
    fresh.close()
    _assert_same_state(got, want)


# ---- hot start through u ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["e226", "structured_lp"])
def test_update_matrix_with_hot_start_equals_fresh_create_with_start(name):
    lp = _ctest(name) if name == "e226" else _lp(name)
    held = _create(lp, updatable="matrix")
    first = held.run(lp.num_col, lp.num_row)
    start = dict(col_value=first.col_value.copy(), row_value=first.row_value.copy(), row_dual=first.row_dual.copy())
    u = MC.modification(lp, "jitter", seed=41)
    lp2 = MC.apply(lp, u)
    held.update_matrix(start=start, **u)
    got = held.run(lp.num_col, lp.num_row)
    fresh = _create(lp2, start=start)
    want = fresh.run(lp.num_col, lp.num_row)
    fresh.close()
    _assert_same_result(got, want)
    # the start is not sticky: the next matrix update without one is a cold start
    held.update_matrix(u["a_value"])
    cold = _create(lp2)
    _assert_same_result(held.run(lp.num_col, lp.num_row), cold.run(lp.num_col, lp.num_row))
    cold.close()
    held.close()


# ---- refusals with a handle leave the solver's bits alone --------------------------------------------------------------
def _refused(ds, *a, **u):
    with pytest.raises(RuntimeError) as e:
        ds.update_matrix(*a, **u)
    return str(e.value)


def test_refused_without_the_matrix_flag():
    lp = _lp("adlittle")
    for flag in (False, True):
        ds, untouched = _create(lp, updatable=flag), _create(lp)
        assert ds.stage("update_state")[4] == 0.0 and ds.stage("update_state")[5] == 0.0  # nothing kept for the matrix
        assert "PDLP_UPDATABLE_MATRIX" in _refused(ds, lp.a_value * 2.0)
        _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
        ds.close(); untouched.close()


def test_refused_for_hipdlp():
    lp = _lp("adlittle")
    ds, untouched = _create(lp, solver="hipdlp", updatable="matrix"), _create(lp, solver="hipdlp")
    assert "HiPDLP" in _refused(ds, lp.a_value * 2.0)
    a, b = ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row)
    for k in SOLUTION:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.num_iter == b.num_iter and a.term_code == b.term_code
    ds.close(); untouched.close()


def test_refused_for_a_sharded_solver(monkeypatch):
    lp = _lp("adlittle")
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    ds, untouched = _create(lp, updatable="matrix"), _create(lp)
    assert "sharded" in _refused(ds, lp.a_value * 2.0)
    _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
    ds.close(); untouched.close()


def test_refused_for_an_off_diagonal_hessian():
    lp = _lp("random_sparse_qp")
    ds, untouched = _create(lp, updatable="matrix"), _create(lp)
    msg = _refused(ds, lp.a_value * 2.0)
    assert "off-diagonal" in msg and "Hessian" in msg
    _assert_same_result(ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row))
    ds.close(); untouched.close()


@pytest.mark.parametrize("name", ["25fv47", "structured_lp"])
def test_refusals_change_nothing(name):
    """A wrong count, NULL values, an all-zero matrix, a row-kind change, a partial start, a lone row bound: each is
    refused with its reason and the solver then iterates exactly as an untouched one (200 iterations)."""
    lp = _lp(name)
    ds, untouched = _create(lp, updatable="matrix"), _create(lp)
    want = _iterate_state(untouched)
    untouched.close()
    a = MC.new_values(lp, 3)
    kind = UC.row_kind(np.asarray(lp.row_lower), np.asarray(lp.row_upper))
    eq = np.nonzero(kind == 0)[0]
    lo, up = np.array(lp.row_lower), np.array(lp.row_upper)
    rows = sorted(int(i) for i in (eq[eq.size // 3], eq[-1]))
    for i in rows:
        up[i] = lo[i] + 1.0  # equality -> ranged
    before = _data(ds)
    assert "num_nz" in _refused(ds, a[:-1])
    assert "a_value is NULL" in _refused(ds, None)
    assert "no matrix nonzeros" in _refused(ds, np.zeros(a.size))
    msg = _refused(ds, a, col_cost=lp.col_cost * 2.0, col_lower=lp.col_lower - 1.0, row_lower=lo, row_upper=up, offset=9.0)
    assert f"row {rows[0]} " in msg and "equality" in msg and "ranged or free" in msg
    assert "partial start" in _refused(ds, a, start=dict(col_value=np.zeros(lp.num_col)))
    assert "row_upper is NULL" in _refused(ds, a, row_lower=lo)
    after = _data(ds)
    for k in DATA:
        assert np.array_equal(before[k], after[k]), k
    _assert_same_state(_iterate_state(ds), want)
    ds.close()


# ---- the flags alone change nothing ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["25fv47", "synthetic_100k", "structured_lp", "dense_column_lp"])
def test_matrix_updatable_solver_never_updated_equals_default(name):
    """Its layouts were built from tagged values and filled by the refill kernels: the same bits as a plain build."""
    lp = _lp(name)
    a, b = _create(lp, updatable="matrix"), _create(lp)
    _assert_same_data(a, b)
    _assert_same_result(a.run(lp.num_col, lp.num_row), b.run(lp.num_col, lp.num_row))
    _assert_same_products(a, b)
    a.close(); b.close()


def test_data_updatable_solver_keeps_what_it_kept():
    """updatable=True (PDLP_UPDATABLE_DATA alone) keeps exactly the memory it kept before matrix updates existed: the pass
    factors 8 * 11 * (n + m) bytes and the row bookkeeping 4 * (2 m + slack columns) bytes.  25fv47 (n = 1571, m = 821, no
    slack column): update_state[0] = 217064 on the commit before this feature, measured there; nothing is reported for
    the matrix."""
    lp = _lp("25fv47")
    ds = _create(lp, updatable=True)
    state = ds.stage("update_state")
    assert state[0] == 88.0 * (ds.n + ds.m) + 4.0 * (2 * ds.m + (ds.n - lp.num_col))
    assert state[0] == PARENT_UPDATE_STATE_25FV47
    assert state[4] == 0.0 and state[5] == 0.0
    ds.close()


PARENT_UPDATE_STATE_25FV47 = 217064.0
