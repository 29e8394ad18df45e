"""pdlp_mi355x_update_values on the device: a held QP solver whose Hessian VALUES are replaced in place (same sparsity
pattern) — alone, or together with new matrix values and data — must be in the state of a fresh pdlp_mi355x_create on the
modified problem with the same `updatable` bits: the same bits in the device's qdiag, N x_start, cost and scale vectors
right after the update, in every solution vector, count and residual after a run, and in the iterates after a fixed
number of iterations.  The oracle is code that exists without this feature: create() on P' built in Python
(tests/update_hessian_cases.py).  No tolerance anywhere, except the reference objective bar of tests/test_gpu_qp.py."""
import copy
import json
import os

import numpy as np
import pytest

import lpgen
import update_hessian_cases as HC
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


def _dense_row_qp():
    """2 000 columns, Q = diag(d) + beta beta' on 600 of them: every row of N in that block has 599 entries, so the N
    operand has long majors and segment tasks."""
    lp = lpgen.drop_free_rows(lpgen.random_lp(4, m=40, n=2000))
    rng = np.random.default_rng(17)
    n = lp.num_col
    block = np.sort(rng.choice(n, 600, replace=False))
    beta = np.zeros(n)
    beta[block] = rng.uniform(0.2, 1.0, 600) * rng.choice([-1.0, 1.0], 600)
    Q = np.outer(beta, beta) + np.diag(rng.uniform(0.1, 2.0, n))
    return lp.set_hessian_from_dense(lp.sense * Q)


def _synthetic_diag_qp():
    sp = solver.SyntheticProblem(40000, 40000, 320000, 3)
    lp = sp.to_lp()
    sp.close()
    return lp.set_diagonal_hessian(np.random.default_rng(7).uniform(0.0, 2.0, lp.num_col))


# name -> (maker, the seed random_sparse_qp was made with or None)
MAKERS = {
    "random_sparse_qp": (lambda: lpgen.random_sparse_qp(3), 3),   # sense = -1
    "bench_qp_banded": (lambda: lpgen.bench_qp_at_scale(200, True), None),
    "dense_row_qp": (_dense_row_qp, None),
    "synthetic_diag_qp": (_synthetic_diag_qp, None),
}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name][0]()
    return _cache[name]


def _create(lp, start=None, **options):
    if start is None:
        return solver.DeviceSolver(lp, **dict(OPTIONS, **options))
    handle = abi.ProblemHandle(lp, start)
    ds = solver.DeviceSolver(problem_struct=handle.struct, **dict(OPTIONS, **options))
    ds._keep = handle
    return ds


def _start(lp, seed=3):
    rng = np.random.default_rng(seed)  # dense: every entry of N takes part in N x_start
    return dict(col_value=rng.uniform(0.5, 1.5, lp.num_col), row_value=rng.standard_normal(lp.num_row),
                row_dual=rng.standard_normal(lp.num_row))


def _vectors(ds, off):
    out = {k: ds.get(k, ds.m if k in ("rhs", "row_scale") else ds.n) for k in DATA}
    out["qdiag"] = ds.get("qdiag", ds.n)
    if off:
        out["nx"] = ds.get("nx", ds.n)
    return out


def _assert_same_vectors(a, b, off=True, zero_off=False):
    va, vb = _vectors(a, off), _vectors(b, off)
    for k in va:
        assert np.array_equal(va[k], vb[k]), k
    if off:  # (N x_start is no trivial zero, unless every value of N is one)
        assert np.any(va["nx"] != 0.0) != zero_off


def _assert_same_result(a, b):
    for k in SOLUTION:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    for k in COUNTS:
        assert getattr(a, k) == getattr(b, k), k
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (k, getattr(a, k), getattr(b, k))


def _iterate_state(ds, iters=200):
    st = ds.iterate(iters)
    out = {k: ds.get(k, ds.m if k in ("y", "ax") else ds.n) for k in ("x", "y", "ax", "aty")}
    out["counts"] = (st.iters, st.trials, st.restarts)
    return out


def _assert_same_state(a, b):
    assert a["counts"] == b["counts"]
    for k in ("x", "y", "ax", "aty"):
        assert np.array_equal(a[k], b[k]), k


def _check_updates(name, kinds, bits, off=True):
    """One held solver; every modification is applied to the ORIGINAL problem with a dense hot start and compared with a
    fresh solver on P' with the same bits and start: the device vectors right after the update, then a whole run."""
    lp = _lp(name)
    held = _create(lp, updatable=bits)
    state = held.stage("update_state")
    assert state[7] == 1.0 and state[6] > 0.0
    graph = state[3]
    start = _start(lp)
    for what in kinds:
        u = HC.modification(lp, what, seed=len(name) + 5, sparse_seed=MAKERS[name][1])
        lp2 = HC.apply(lp, u)
        held.update_values(start=start, **u)
        if "a_value" not in u:  # a Hessian-only update keeps the captured graph
            assert held.stage("update_values_seconds")[4] == 0.0 and held.stage("update_state")[3] == graph
        fresh = _create(lp2, start=start, updatable=bits)
        _assert_same_vectors(held, fresh, off, zero_off=what == "zero_off")
        _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
        fresh.close()
    held.close()


# ---- 1, 3, 6: Hessian-only updates; 2, 3: with a_value and data ----------------------------------------------------------
@pytest.mark.parametrize("slab", ["0", "1"])
@pytest.mark.parametrize("name", ["random_sparse_qp", "bench_qp_banded", "dense_row_qp"])
def test_hessian_only_update_equals_fresh_create(name, slab, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", slab)
    _check_updates(name, ("scale0.3", "scale7", "regen", "diag_only", "zero_off"), "hessian")


@pytest.mark.parametrize("slab", ["0", "1"])
@pytest.mark.parametrize("name", ["random_sparse_qp", "bench_qp_banded", "dense_row_qp"])
def test_update_values_with_matrix_and_data_equals_fresh_create(name, slab, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", slab)
    _check_updates(name, ("all",), "matrix+hessian")


def test_update_values_without_scaling():
    """Nothing is replayed: the assembled values are the scaled ones."""
    _check_updates_kw = dict(pdlp_features_off=abi.FEATURE_SCALING_OFF)
    lp = _lp("bench_qp_banded")
    for bits, what in (("hessian", "regen"), ("matrix+hessian", "all")):
        u = HC.modification(lp, what, seed=9)
        held = _create(lp, updatable=bits, **_check_updates_kw)
        held.update_values(start=_start(lp), **u)
        fresh = _create(HC.apply(lp, u), start=_start(lp), updatable=bits, **_check_updates_kw)
        _assert_same_vectors(held, fresh)
        _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
        held.close(); fresh.close()


# ---- 4: a diagonal QP prepared on the device, the fused loop, the captured graph kept --------------------------------------
def test_diagonal_qp_from_the_device_setup_keeps_its_graph(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1")
    lp = _lp("synthetic_diag_qp")
    assert lp.num_nz >= 200_000  # the device-side set-up
    held = _create(lp, updatable="hessian")
    assert held.stage("trial_launches")[0] == 2.0  # the fused form
    assert held.stage("update_state")[3] == 1.0
    u = HC.modification(lp, "regen", seed=3)
    held.update_values(**u)
    secs = held.stage("update_values_seconds")
    assert secs[4] == 0.0 and held.stage("update_state")[3] == 1.0  # graphExec_ is the one captured at create
    fresh = _create(HC.apply(lp, u), updatable="hessian")
    _assert_same_vectors(held, fresh, off=False)
    _assert_same_state(_iterate_state(held), _iterate_state(fresh))
    held.close(); fresh.close()


# ---- 5: a chain on one solver ----------------------------------------------------------------------------------------------
def test_chain_of_hessian_and_matrix_updates_on_one_solver():
    lp = _lp("bench_qp_banded")
    q0 = np.array(lp.hessian[2])
    a1 = MC.new_values(lp, 23, ("jitter", "decades"))
    steps = [dict(q_value=1.0 * q0), dict(q_value=0.3 * q0), dict(q_value=7.0 * q0), dict(a_value=a1),
             dict(a_value=np.array(lp.a_value), q_value=1.0 * q0)]
    held = _create(lp, updatable="matrix+hessian")
    target, results = lp, []
    for u in steps:
        held.update_values(**u)
        target = HC.apply(target, u)
        results.append(held.run(lp.num_col, lp.num_row))
        fresh = _create(target, updatable="matrix+hessian")
        _assert_same_result(results[-1], fresh.run(lp.num_col, lp.num_row))
        fresh.close()
    held.close()
    _assert_same_result(results[0], results[-1])


# ---- 7: update_matrix on a Hessian-updatable off-diagonal QP -----------------------------------------------------------------
def test_update_matrix_of_an_off_diagonal_qp_is_accepted_with_the_hessian_bit():
    lp = _lp("random_sparse_qp")
    u = MC.modification(lp, "all", seed=29)
    held = _create(lp, updatable="matrix+hessian")
    held.update_matrix(start=_start(lp), **u)
    fresh = _create(MC.apply(lp, u), start=_start(lp), updatable="matrix+hessian")
    _assert_same_vectors(held, fresh)
    _assert_same_result(held.run(lp.num_col, lp.num_row), fresh.run(lp.num_col, lp.num_row))
    held.close(); fresh.close()


# ---- 8: refusals leave a 200-iteration state alone --------------------------------------------------------------------------
def _refused(ds, **u):
    with pytest.raises(RuntimeError) as e:
        ds.update_values(**u)
    return str(e.value)


def test_refusals_change_nothing():
    lp = _lp("random_sparse_qp")
    q = np.array(lp.hessian[2])
    st, idx, _ = lp.hessian
    cols = np.repeat(np.arange(len(st) - 1), np.diff(st))
    diag = np.nonzero(np.asarray(idx) == cols)[0]
    bad = q.copy()
    for p in (diag[-1], diag[1]):
        bad[p] = -lp.sense * 0.25
    ds, untouched = _create(lp, updatable="matrix+hessian"), _create(lp, updatable="matrix+hessian")
    want = _iterate_state(untouched)
    untouched.close()
    before = _vectors(ds, True)
    assert "num_q_nz" in _refused(ds, q_value=q[:-1])
    msg = _refused(ds, q_value=bad, a_value=2.0 * lp.a_value, col_cost=2.0 * lp.col_cost)
    assert "not positive semidefinite for this objective sense" in msg and f"column {int(cols[diag[1]])} " in msg
    assert "num_nz" in _refused(ds, q_value=2.0 * q, a_value=lp.a_value[:-1])
    assert "partial start" in _refused(ds, q_value=2.0 * q, start=dict(col_value=np.zeros(lp.num_col)))
    after = _vectors(ds, True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    _assert_same_state(_iterate_state(ds), want)
    ds.close()


def test_refusal_precedence_is_the_host_twins():
    """Doubly wrong updates (HC.doubly_wrong): the device refuses with the words of pdlp_mi355x_host_prepare_qp, in its
    order — row kind, all-zero matrix, Hessian diagonal — and writes nothing."""
    lp = _lp("random_sparse_qp")
    ds, untouched = _create(lp, updatable="matrix+hessian"), _create(lp, updatable="matrix+hessian")
    want = _iterate_state(untouched)
    untouched.close()
    before = _vectors(ds, True)
    for name, (u, words) in HC.doubly_wrong(lp).items():
        data = {k: v for k, v in u.items() if k not in ("a_value", "q_value")}
        with pytest.raises(RuntimeError) as host:
            solver.host_prepare_qp(lp, a_value=u.get("a_value"), q_value=u.get("q_value"),
                                   update=abi.UpdateHandle(**data) if data else None, updatable="matrix+hessian")
        # (the Python layer puts "<entry> failed: " in front of the library's message, on either side)
        msg, twin = _refused(ds, **u).split(" failed: ", 1)[1], str(host.value).split(" failed: ", 1)[1]
        assert words in msg and msg == twin, (name, msg, twin)
    after = _vectors(ds, True)
    for k in before:
        assert np.array_equal(before[k], after[k]), k
    _assert_same_state(_iterate_state(ds), want)
    ds.close()


@pytest.mark.parametrize("why", ["missing_bit", "matrix_bit_only", "lp", "hipdlp", "sharded"])
def test_refused_by_how_the_solver_was_created(why, monkeypatch):
    lp = _lp("random_sparse_qp")
    q = 2.0 * np.array(lp.hessian[2])
    if why == "lp":
        lp = lpgen.random_lp(5)
        q = np.ones(3)
    if why == "sharded":
        monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    options = dict(missing_bit=dict(updatable=True), matrix_bit_only=dict(updatable="matrix"), lp=dict(updatable="hessian"),
                   hipdlp=dict(updatable="hessian", solver="hipdlp"), sharded=dict(updatable="hessian"))[why]
    words = dict(missing_bit="PDLP_UPDATABLE_HESSIAN", matrix_bit_only="PDLP_UPDATABLE_HESSIAN", lp="created without a Hessian",
                 hipdlp="HiPDLP", sharded="sharded")[why]
    if why == "hipdlp":
        lp = lpgen.random_lp(5)  # (the HiPDLP path takes LPs only)
    ds, untouched = _create(lp, **options), _create(lp, **options)
    assert words in _refused(ds, q_value=q)
    a, b = ds.run(lp.num_col, lp.num_row), untouched.run(lp.num_col, lp.num_row)
    for k in SOLUTION:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.num_iter == b.num_iter and a.term_code == b.term_code
    ds.close(); untouched.close()


# ---- 9: unchanged create paths -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random_sparse_qp", "bench_qp_banded", "dense_row_qp"])
def test_hessian_updatable_solver_never_updated_equals_default(name):
    """Its N operand was built from tagged values and filled by the refill kernel: the same bits as a plain build (these
    patterns hold no explicit zero, so the pattern contract changes nothing)."""
    lp = _lp(name)
    assert np.all(np.asarray(lp.hessian[2]) != 0.0)
    start = _start(lp)
    a, b = _create(lp, start=start, updatable="hessian"), _create(lp, start=start)
    _assert_same_vectors(a, b)
    _assert_same_result(a.run(lp.num_col, lp.num_row), b.run(lp.num_col, lp.num_row))
    a.close(); b.close()


# update_state[0] and [4] of tests/golden/instances/25fv47 on the commit before this feature, measured there
PARENT_UPDATE_STATE_25FV47 = {0: (0.0, 0.0), True: (217064.0, 0.0), "matrix": (217064.0, 559344.0)}


@pytest.mark.parametrize("bits", [0, True, "matrix"])
def test_solvers_without_the_bit_keep_what_they_kept(bits):
    lp = L.HighsLp.from_npz(os.path.join(GOLD, "instances", "25fv47.npz"))
    ds = _create(lp, updatable=bits)
    state = ds.stage("update_state")
    want = PARENT_UPDATE_STATE_25FV47[bits]
    assert state[0] == want[0] and state[4] == want[1]
    assert state[5] == (1.0 if bits == "matrix" else 0.0)
    assert state[6] == 0.0 and state[7] == 0.0  # nothing is kept for the Hessian
    ds.close()


# ---- 10: tie to the reference ------------------------------------------------------------------------------------------------
REF_SPARSE = json.load(open(os.path.join(GOLD, "reference_qp_sparse.json")))


@pytest.mark.parametrize("name", ["sq0", "qjh_mps"])
def test_update_values_reaches_the_reference_optimum(name):
    lp = L.HighsLp.from_npz(os.path.join(GOLD, "qp", name + ".npz"))
    twice = copy.copy(lp)
    twice.hessian = (lp.hessian[0], lp.hessian[1], 2.0 * np.asarray(lp.hessian[2], dtype=np.float64))
    ds = solver.DeviceSolver(twice, updatable="hessian", kkt_tolerance=1e-8, pdlp_iteration_limit=2000000)
    ds.update_values(q_value=lp.hessian[2])
    out = ds.solve()
    ds.close()
    assert out.model_status == solver.kOptimal
    ref = REF_SPARSE[name]["objective_value"]
    assert abs(out.info["objective_function_value"] - ref) <= 1e-6 * (1 + abs(ref))
