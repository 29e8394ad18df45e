"""What tests/test_gpu_check_stats.py relies on, shown without a GPU on tests/check_cases.py alone: the generated problems have
the promised structure, the planted states reach every branch of the statistics a guaranteed number of times, integer data
keep every term and every sum an exact double, the any-order bound is not vacuous on real data, and the reference's derived
numbers reproduce a 3 x 3 example worked by hand.  The averages are restated as the check computes them on a fresh solver
(sumPrimalStep = 0: x_avg = x_sum, ax_avg = A x_sum, aty_avg = A' y_sum).

The 3 x 3 example (formulated, unscaled; one equality row, then two inequality rows):
    c = (1, -2, 3)     column 0: x >= 0, column 1: free, column 2: -1 <= x <= 2          b = (1, 2, -1)
    x = (2, -1, 1)     ax = (1, 1, 0)     y = (1, -1, 2)     aty = (0, -3, 5)     (ax, aty as stored: not A x, A' y)
  rows     ax - b = (0, -1, 1), projected on the inequality rows (0, -1, 0): 1;  y'b = 1 - 2 - 2 = -3;  ||y||^2 = 6;
           ray (1, min(1, 0), min(0, 0)): 1
  columns  c'x = 2 + 2 + 3 = 7;  r = c - aty = (1, 1, -2);  s+ = (1, 0, 0) (column 1 has no lower bound);  s- = (0, 0, 2);
           s+'l = 0;  s-'u = 4;  r - s+ + s- = (0, 1, 0): 1;  ||s+||^2 = 1;  ||s-||^2 = 4;  aty + s+ - s- = (1, -3, 3): 19;
           ||x||^2 = 6;  min(x, 0) hasL = (0, 0, 0): 0;  max(x, 0) hasU = (0, 0, 1): 1
  derived  primal_obj 7, dual_obj -3 + 0 - 4 = -7, primal_feas 1, dual_feas 1, gap 14, rel. gap 14 / 15,
           ||(y, s+, s-)|| = sqrt(11): ray objective -7 / sqrt(11), ray residual sqrt(19 / 11) (as sqrt(19) / sqrt(11));
           ||x|| = sqrt(6): 7 / sqrt(6) and sqrt(2) / sqrt(6).  With sense -1 and offset 10: primal_obj 3, dual_obj 17."""
import math

import numpy as np
import pytest

import check_cases as K
import edge_cases as E
from highs_amd import solver

INF = K.INF
_prepared = {}


def _form(lp, values):
    """(Prepared, scaled) of a problem as the device will hold it: integer cases without scaling."""
    key = (lp.model_name, values)
    if key not in _prepared:
        _prepared[key] = solver.Prepared(lp, **(dict(pdlp_features_off=1) if values == "integer" else {}))
    return _prepared[key], values != "integer"


def _state(P, values, seed, data=None, qp=None):
    """Held data + planted vectors + the averages of a fresh solver, as tests/test_gpu_check_stats.py reads them back."""
    rng = np.random.default_rng(seed)
    v = dict(cost=P.cost, rhs=P.rhs, lower=P.lower, upper=P.upper, col_scale=P.col_scale, row_scale=P.row_scale)
    if data:
        v.update(K.planted_data(P.n, P.m, values, rng))
    if qp is not None:
        v["qdiag"] = qp
    v.update(K.planted(dict(cost=v["cost"], rhs=v["rhs"], qdiag=v.get("qdiag")), values, rng))
    v["x_avg"], v["y_avg"] = v["x_sum"], v["y_sum"]
    rows, cols = np.repeat(np.arange(P.m), np.diff(P.csr_beg)), np.repeat(np.arange(P.n), np.diff(P.csc_beg))
    v["ax_avg"] = np.bincount(rows, weights=P.csr_val * v["x_avg"][P.csr_idx], minlength=P.m)
    v["aty_avg"] = np.bincount(cols, weights=P.csc_val * v["y_avg"][P.csc_idx], minlength=P.n)
    return v


def _assert_classes_filled(v, n_eqs, name, zero_r=True):
    classes = K.branch_classes(v, n_eqs)
    n_ineq = len(v["rhs"]) - n_eqs
    for what, mask in classes.items():
        if not zero_r and "r = 0" in what:
            continue
        population = n_ineq if what.startswith("row") else len(v["cost"])
        assert mask.sum() >= max(1, math.ceil(0.01 * population)), (name, what, int(mask.sum()), population)
        assert mask[-256:].any(), (name, what, "none in the last 256 indices")


SIZED = [(n, m, thin) for n, m in K.SIZES[1:] for thin in ((False, True) if (n, m) == (65537, 300) else (False,))]


@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("n,m,thin", SIZED)
def test_generated_problems_and_planted_states(n, m, thin, values):
    lp = K.sized_lp(n, m, values, thin=thin)
    P, scaled = _form(lp, values)
    # the formulation keeps the problem as generated: same columns, equality rows first, no row negated, no column added
    assert (P.n, P.m, P.n_eqs) == (n, m, m // 2) and 0 < P.n_eqs < m
    per_col = P.nnz / n
    assert (0.2 < per_col < 0.3) if thin else (1.9 < per_col <= 2.0)
    kinds = [(np.isfinite(P.lower[k::5]).all(), np.isfinite(P.upper[k::5]).all(), np.isinf(P.lower[k::5]).all(), np.isinf(P.upper[k::5]).all())
             for k in range(5)]
    assert kinds == [(False, False, True, True), (True, False, False, True), (False, True, True, False), (True, True, False, False),
                     (True, True, False, False)]
    assert np.all(P.lower[3::5] < P.upper[3::5]) and np.array_equal(P.lower[4::5], P.upper[4::5])
    if values == "integer":
        assert np.array_equal(P.cost, lp.col_cost) and np.array_equal(P.rhs, lp.row_lower) and np.array_equal(P.lower, lp.col_lower)
        for a in (P.cost, P.rhs, P.csr_val, P.lower[np.isfinite(P.lower)], P.upper[np.isfinite(P.upper)]):
            assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= 8
    v = _state(P, values, seed=5)
    _assert_classes_filled(v, P.n_eqs, lp.model_name)
    ref = K.reference_stats(v, P.n_eqs, scaled, integer=(values == "integer"))
    assert len(ref["q"]) == K.N_STATS == len(K.NAMES) == 30
    _assert_reference_is_sound(ref, values, lp.model_name)
    # the average half sees both signs of every residual too (it cannot be planted: the check computes it)
    avg = K.branch_classes(v, P.n_eqs, "avg")
    for what in ("row: ax - b < 0", "row: ax - b > 0", "col: r < 0, lower", "col: r > 0, upper", "col: x < 0, lower", "col: x > 0, upper"):
        assert avg[what].sum() >= 0.01 * (m - P.n_eqs if what.startswith("row") else n), what


def _assert_reference_is_sound(ref, values, name):
    for k, q in enumerate(ref["q"]):
        if values == "integer":
            # every partial sum of the terms, in any order, is an integer (a half-integer) of magnitude below 2^53: exact
            assert q.abs_sum < 2.0**53, (name, K.NAMES[k], q.abs_sum)
            scale = 2 if K.NAMES[k].startswith("half_xqx") else 1
            assert np.array_equal(q.terms * scale, (q.terms * scale).astype(np.int64)) and q.fsum * scale == q.exact, (name, K.NAMES[k])
        else:
            # numpy's pairwise sum is one of the orders the bound covers — and it does not always hit the rounded exact sum:
            # the bound is needed, and it holds
            assert abs(float(np.sum(q.terms)) - q.fsum) <= K.any_order_bound(q), (name, K.NAMES[k])
    if values == "real":
        assert any(float(np.sum(q.terms)) != q.fsum for q in ref["q"] if q.length > 256) or all(q.length <= 256 for q in ref["q"])
        assert all(K.any_order_bound(q) <= 1e-9 * max(q.abs_sum, 1e-300) for q in ref["q"])  # (a bound of 1e-9 relative at most)


@pytest.mark.parametrize("qp", ["diag", "sparse"])
@pytest.mark.parametrize("values", ["integer", "real"])
def test_qp_terms_stay_exact_on_integer_data(values, qp):
    n, m = 65537, 300
    lp = K.sized_lp(n, m, values, qp=qp)
    st, idx, val = lp.hessian
    cols = np.repeat(np.arange(n), np.diff(st))
    diag = np.zeros(n)
    diag[idx[idx == cols]] = val[idx == cols]
    assert (idx != cols).sum() == (0 if qp == "diag" else (np.arange(n - 3) % 7 == 0).sum()) and np.all(diag > 0)
    if values == "integer":
        assert np.array_equal(diag % 2, np.zeros(n)) and np.abs(val).max() <= 8 and np.array_equal(val, np.rint(val))
    P, scaled = _form(lp, values)
    rng = np.random.default_rng(6)
    v = dict(cost=P.cost, rhs=P.rhs, lower=P.lower, upper=P.upper, col_scale=P.col_scale, row_scale=P.row_scale, qdiag=diag)
    v.update(K.planted(dict(cost=P.cost, rhs=P.rhs, qdiag=diag, nx=(qp == "sparse")), values, rng))
    v["x_avg"], v["y_avg"], v["ax_avg"], v["aty_avg"] = v["x"], v["y"], v["ax"], v["aty"]  # (any vectors serve here)
    if qp == "sparse":
        v["nx_avg"] = v["nx"]
    _assert_classes_filled(v, P.n_eqs, lp.model_name, zero_r=(values == "integer"))
    ref = K.reference_stats(v, P.n_eqs, scaled, integer=(values == "integer"))
    assert ref["qp"]
    _assert_reference_is_sound(ref, values, lp.model_name)
    half = ref["q"][8 + K.COL_STATS - 1]
    assert half.abs_sum > 0
    if values == "integer" and qp == "sparse":
        assert np.any(half.terms != np.rint(half.terms)) and half.exact % 2 in (0, 1)  # half-integers occur, and are exact


@pytest.mark.parametrize("name,g", [("grid32", 32), ("grid33", 33), ("grid64", 64), ("grid65", 65), ("wide16385", 64)])
@pytest.mark.parametrize("values", ["integer", "real"])
def test_planted_data_on_the_edge_cases(name, g, values):
    """The grid cases and wide(16385) of tests/edge_cases.py (boxed columns, `<=` rows, real costs) with planted data and
    states: the same guarantees.  g: workgroups of the persistent loop (the one-launch check takes at most 64; at 16385
    columns the 65 virtual blocks of the column statistics share 64 workgroups)."""
    lp = E.wide(16385, values) if name == "wide16385" else E.grid(g, values)
    P, scaled = _form(lp, values)
    assert P.n_eqs == 0 and max(solver.stream_plan(P, 0)["small_grid"], solver.stream_plan(P, 1)["small_grid"]) == g
    v = _state(P, values, seed=7, data=True)
    _assert_classes_filled(v, 0, lp.model_name)
    _assert_reference_is_sound(K.reference_stats(v, 0, scaled, integer=(values == "integer")), values, lp.model_name)


def test_the_thin_matrix_fits_the_one_launch_check():
    """At most 64 workgroups, as the device set-up will find (the loop's grid is the larger of the two operands')."""
    for values in ("integer", "real"):
        P, _ = _form(K.sized_lp(65537, 300, values, thin=True), values)
        a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
        assert a["chunk"] == at["chunk"] == 512 and max(a["small_grid"], at["small_grid"]) == 64, (a["small_grid"], at["small_grid"])
        assert max(a["n_blocks"], at["n_blocks"]) <= 64 and -(-65537 // 256) == 257 > 64
        P, _ = _form(K.sized_lp(65537, 300, values), values)
        assert max(solver.stream_plan(P, 0)["small_grid"], solver.stream_plan(P, 1)["small_grid"]) > 64


def test_smallest_problem():
    lp = K.sized_lp(1, 1, "integer")
    P, _ = _form(lp, "integer")
    assert (P.n, P.m, P.nnz, P.n_eqs) == (1, 1, 1, 0)
    v = _state(P, "integer", seed=5)
    ref = K.reference_stats(v, 0, False, integer=True)
    assert all(q.length == 1 and q.fsum == q.terms[0] for q in ref["q"])


def test_derived_numbers_on_the_worked_example():
    v = dict(cost=np.array([1.0, -2.0, 3.0]), lower=np.array([0.0, -INF, -1.0]), upper=np.array([INF, INF, 2.0]),
             rhs=np.array([1.0, 2.0, -1.0]), x=np.array([2.0, -1.0, 1.0]), ax=np.array([1.0, 1.0, 0.0]), y=np.array([1.0, -1.0, 2.0]),
             aty=np.array([0.0, -3.0, 5.0]))
    for k in ("x", "y", "ax", "aty"):
        v[k + "_avg"] = v[k]
    ref = K.reference_stats(v, 1, False, integer=True)
    sums = K.exact_values(ref)
    assert sums[:4].tolist() == [1, -3, 6, 1] and sums[8:19].tolist() == [7, 0, 4, 1, 1, 4, 19, 6, 0, 1, 0]
    assert np.array_equal(sums[4:8], sums[:4]) and np.array_equal(sums[19:], sums[8:19])
    assert ref["slack_pos"].tolist() == [1, 0, 0] and ref["slack_neg"].tolist() == [0, 0, 2]
    d = dict(zip(K.DERIVED_NAMES, K.derived(sums, False)))
    assert (d["pObj"], d["dObj"], d["pFeas"], d["dFeas"], d["gap"]) == (7.0, -7.0, 1.0, 1.0, 14.0)
    assert d["relGap"] == 14.0 / 15.0
    assert d["pInfObj"] == -7.0 / math.sqrt(11.0) and d["pInfRes"] == math.sqrt(19.0) / math.sqrt(11.0)
    assert d["dInfObj"] == 7.0 / math.sqrt(6.0) and d["dInfRes"] == math.sqrt(2.0) / math.sqrt(6.0)
    d = K.derived(sums, False, sense=-1.0, offset=10.0)
    assert (d[0], d[1], d[10], d[11]) == (3.0, 17.0, 3.0, 17.0) and d[6] == -7.0 / math.sqrt(11.0) and d[8] == 7.0 / math.sqrt(6.0)
    # both scales fall back to 1 below 1e-8; a QP moves 1/2 x'Qx from the dual to the primal objective
    z = np.zeros(30)
    z[8], z[9] = 2.0, 3.0
    d = K.derived(z, False)
    assert (d[0], d[1], d[6], d[8]) == (2.0, 3.0, 3.0, 2.0)
    z[18] = 0.5
    assert K.derived(z, True)[:2].tolist() == [2.5, 2.5]
