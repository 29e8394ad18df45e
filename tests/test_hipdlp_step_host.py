"""What tests/test_gpu_hipdlp_step.py relies on, proven without a GPU (cases, plans and numbers: tests/hipdlp_step_cases.py):
  - every edge case keeps its pattern and its integer values through HiPDLP's formulation (the oracle's), with no slack
    column, no reordered row and no scaling;
  - the stream layout, the slab layout's long majors and the rule of the persistent step launch make of each case what the
    table hipdlp_step_cases.EXPECT says (solver.stream_plan and the host-only hook of halpernSmallReason);
  - the two planted starts of each case put every marked major — more than 256 entries, first or last of a work block, or in
    a work block without entries — strictly inside its bounds (plan "free") and on or beyond one (plan "clamped"), seen from the
    restatement's own temp, and both products of two steps are exact in any summation order;
  - the restatement itself, by hand on a 2 x 2 problem."""
import numpy as np
import pytest

import hipdlp_check_cases as H
import hipdlp_step_cases as SC
from test_hipdlp_small_host import rule

INF = H.INF


# ---- the form -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_formulation_keeps_pattern_and_integer_values(name):
    lp, F = SC.case_lp(name, "integer"), SC.formulated(name)
    assert (F.n, F.m, F.n_eqs) == (lp.num_col, lp.num_row, 0)
    A = F.A.tocsc()
    A.sort_indices()
    assert np.array_equal(A.indptr, lp.a_start) and np.array_equal(A.indices, lp.a_index)
    assert np.array_equal(A.data, -np.asarray(lp.a_value))  # (every row is a `<=` row: negated into `>=`)
    assert np.array_equal(A.data, np.rint(A.data)) and np.abs(A.data).min() >= 1 and np.abs(A.data).max() <= 8
    assert np.all(F.col_scale == 1.0) and np.all(F.row_scale == 1.0)
    assert np.all(np.isfinite(F.rhs)) and np.all(F.row_upper == INF)
    assert np.array_equal(F.lower, np.zeros(F.n)) and np.array_equal(F.upper, np.ones(F.n))
    assert not np.array_equal(F.cost, np.rint(4.0 * F.cost) / 4.0)  # the cost stays real: the tests plant it


# ---- the table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SC.CASES))
def test_planners_and_rule_give_the_table(name):
    a, at, slab_a, slab_at = SC.plans(name)
    ex = SC.EXPECT[name]
    assert (a["chunk"], at["chunk"]) == (ex.chunk, ex.chunk)
    assert (a["n_blocks"], a["n_long"], a["n_tasks"]) == ex.a and (at["n_blocks"], at["n_long"], at["n_tasks"]) == ex.at
    assert (slab_a["n_long"], slab_at["n_long"]) == ex.slab
    assert (slab_a["long_group"], slab_at["long_group"]) == (ex.group, 1) and a["long_group"] == at["long_group"] == 1
    F = SC.formulated(name)
    for M, plan, slab in ((F.A.tocsr(), a, slab_a), (F.A.tocsc(), at, slab_at)):
        lens = np.diff(M.indptr)
        assert np.array_equal(plan["long_majors"], np.nonzero(lens > ex.chunk)[0])
        assert np.array_equal(slab["long_majors"], np.nonzero(lens > SC.LONG)[0])
    capped = tuple((int((p["blocks"][:, 1] - p["blocks"][:, 0] == 2048).sum()), int((p["blocks"][:, 2] == p["blocks"][:, 3]).sum())) for p in (a, at))
    assert capped == SC.CAPPED.get(name, ((0, 0), (0, 0)))
    got = rule(**SC.rule_shape(name))
    assert (got if got[0] == 0 else got[0]) == ex.rule
    if got[0] == 0:  # without the XCD-local mode: agent scope whatever the grid
        assert rule(0, **SC.rule_shape(name)) == (0, got[1], 0)
    assert (name in SC.PERSISTENT_CASES) == (got[0] == 0)
    assert rule(**dict(SC.rule_shape(name), use_slab=1))[0] == 4  # the slab layout keeps the plain launches


def test_table_rows_by_number():
    """The same table, spelled out once more where a number is the point of the case."""
    P = {name: SC.plans(name) for name in SC.CASES}
    assert [P[k][2]["n_long"] for k in ("long2048", "long2049")] == [2048, 2049]
    assert [P[k][2]["long_group"] for k in ("long2048", "long2049")] == [1, 2]
    assert [P[k][2]["long_slots"] for k in ("long2048", "long2049")] == [2048, 1025]
    assert P["segments"][0]["n_tasks"] == 118 and P["limit2048"][0]["n_tasks"] == 5 and P["limit512"][1]["n_tasks"] == 2
    assert [rule(**SC.rule_shape("grid%d" % g)) for g in (32, 33, 64)] == [(0, 32, 1), (0, 33, 0), (0, 64, 0)]
    assert rule(**SC.rule_shape("grid65"))[0] == 7
    assert rule(**SC.rule_shape("wide10000")) == (0, 8, 1) and rule(**SC.rule_shape("wide16385")) == (0, 11, 1)
    # blocks without entries own majors all the same: the columns 2556 .. 4603 of empty_runs, the last 12801 columns of wide16385
    assert P["empty_runs"][1]["blocks"].tolist()[2] == [2556, 4604, 516, 516]
    assert P["empty_runs4600"][0]["blocks"].tolist()[1] == [2048, 4096, 3, 3]
    b = P["wide16385"][1]["blocks"]
    assert [int(r[1] - r[0]) for r in b if r[2] == r[3]] == [2048] * 6 + [513] and b[-1, 1] == 16385  # (column 16384 is the block's last major)


# ---- the planted starts -------------------------------------------------------------------------------------------------------
def _assert_plan(name, plan_name, sigma, h_iter, dyadic, steps):
    F = SC.formulated(name)
    rows, cols = SC.marked(name)
    assert rows.any() and cols.any()
    d = SC.step_data(name, plan_name, np.random.default_rng(23), sigma=sigma, dyadic_anchors=dyadic)
    assert np.array_equal(d["cost"], np.rint(4.0 * d["cost"]) / 4.0) and np.all(d["cost"] != 0.0)
    kinds = (np.isinf(d["row_upper"]), d["rhs"] == d["row_upper"], (d["rhs"] < d["row_upper"]) & np.isfinite(d["row_upper"]))
    assert np.all(kinds[0] | kinds[1] | kinds[2])
    few_rows = int((~rows).sum()) < 33  # (segments, grid*, wide*: every row is marked, and its bounds are the plan's)
    assert few_rows or all(k[~rows].any() for k in kinds)
    want, trace = SC.restate(name, d, steps, sigma, h_iter)
    A, At = F.A.tocsr(), F.A.T.tocsr()
    for s, tr in enumerate(trace):
        for M, v in ((At, tr["aty_operand"]), (A, tr["ax_operand"])):
            g, units = SC.exact_units(M, v)
            assert units < 2.0**53, (name, plan_name, s, g, units)
    first = trace[0]
    if steps == 2:  # the second step is not planned; some marked major carries its sum there all the same (unclamped column, clamped row)
        assert (trace[1]["col_class"][cols] == 0).any() and (trace[1]["row_class"][rows] != 0).any()
    cc, rc = first["col_class"][cols], first["row_class"][rows]
    if plan_name == "free":
        assert np.all(cc == 0) and np.all(rc == 0)
    else:
        assert np.all(cc != 0) and np.all(rc != 0)
        assert (np.abs(cc) == 2).any() and (np.abs(rc) == 2).any()  # exactly on a bound
        assert (cc == -1).any() and (cc == 1).any() and (rc == -1).any() and (rc == 1).any()
    # the whole problem reaches every class of both projections in the first step
    assert set(np.unique(first["col_class"])) == {-2, -1, 0, 1, 2}
    lo, up = d["lower"], d["upper"]
    neg0 = ((lo == 0) & np.signbit(lo)) | ((up == 0) & np.signbit(up))
    assert ((first["temp"] == 0) & neg0).any() and (lo == up).any() and (lo == -INF).any() and (up == INF).any()
    on_l, on_u = first["temp_y"] == -d["rhs"], first["temp_y"] == -d["row_upper"]
    assert few_rows or (on_l[~rows].any() and on_u[~rows].any())
    return first, rows, cols, on_u


@pytest.mark.parametrize("plan_name", SC.PLANS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_two_dyadic_steps_are_exact_and_every_marked_major_is_in_its_class(name, plan_name):
    """tau = 1/4, sigma = 2, hIter = 0, dyadic anchors: the operands of A'y and of A x_reflected of steps 1 and 2."""
    _assert_plan(name, plan_name, 2.0, 0, True, 2)


@pytest.mark.parametrize("plan_name", SC.PLANS)
@pytest.mark.parametrize("name", list(SC.CASES))
def test_one_real_step_has_exact_products_and_the_same_classes(name, plan_name):
    """sigma = 0.37, hIter = 7, real anchors: the one step's two products are exact, the classes hold."""
    _assert_plan(name, plan_name, 0.37, 7, False, 1)


@pytest.mark.parametrize("name", list(SC.CASES))
def test_over_the_two_plans_every_marked_major_is_free_once_and_clamped_once(name):
    rows, cols = SC.marked(name)
    seen = {}
    for plan_name in SC.PLANS:
        d = SC.step_data(name, plan_name, np.random.default_rng(23))
        _, trace = SC.restate(name, d, 1, 2.0, 0)
        seen[plan_name] = (trace[0]["row_class"][rows], trace[0]["col_class"][cols])
    for k in (0, 1):
        assert np.all(seen["free"][k] == 0) and np.all(seen["clamped"][k] != 0)
    F = SC.formulated(name)
    for M, mask in ((F.A.tocsr(), rows), (F.A.tocsc(), cols)):
        assert np.all(mask[np.diff(M.indptr) > SC.LONG])  # every long major is marked


def test_exact_units():
    import scipy.sparse as sp
    A = sp.csr_matrix(np.array([[1.0, -2.0, 0.0], [0.0, 0.0, 3.0], [0.0, 0.0, 0.0]]))
    assert SC.exact_units(A, np.array([0.25, -0.5, 1.0])) == (0.25, 12.0)  # row 0: 1 + 4 = 5 units, row 1: 3 x 4 = 12
    assert SC.exact_units(A, np.array([2.0, 4.0, 6.0])) == (1.0, 18.0)
    assert SC.grid_of(np.array([0.0, 3.0 / 32.0])) == 1.0 / 32.0
    with pytest.raises(AssertionError):
        SC.grid_of(np.array([0.1]))


# ---- the restatement by hand --------------------------------------------------------------------------------------------------
def _hand(x, rhs, row_upper):
    import scipy.sparse as sp
    A = sp.csc_matrix(np.array([[1.0, 2.0], [3.0, 4.0]]))
    d = dict(x=np.array(x), y=np.array([4.0, -4.0]), x_anchor=np.array([3.0, 6.0]), y_anchor=np.array([2.0, -2.0]), cost=np.array([-4.0, 4.0]),
             lower=np.array([0.0, 0.0]), upper=np.array([0.5, 5.0]), rhs=np.array(rhs), row_upper=np.array(row_upper))
    return A, d


def test_halpern_step_by_hand_clamped_branches():
    """A = [1 2; 3 4], y = (4, -4): A'y = (-8, -8), c - A'y = (4, 12), tau (c - A'y) = (1, 3).
    x = (2, 2): temp = (1, -1); column 0 in [0, 1/2] is above (proj 1/2), column 1 in [0, 5] below (proj 0);
    slack = (proj - temp) / tau = (-2, 4); x_reflected = 2 proj - x = (-1, -2); A x_reflected = (-5, -11);
    temp_y = y / 2 - A x_reflected = (7, 9).  Row 0: rl = -5, ru = inf, so [-inf, 5]: above, proj_y = 5, dual = (7 - 5) 2 = 4.
    Row 1: rl = -20, ru = -12, so [12, 20]: below, proj_y = 12, dual = (9 - 12) 2 = -6.  y_reflected = 2 dual - y = (4, -8).
    k = 1: w = 1/2; x = (-1 + 3, -2 + 6) / 2 = (1, 2); y = (4 + 2, -8 - 2) / 2 = (3, -5)."""
    A, d = _hand([2.0, 2.0], [-5.0, -20.0], [INF, -12.0])
    temp = H.halpern_step(A, d, 0.25, 2.0, 0, 1, True)
    assert temp.tolist() == [1.0, -1.0]
    assert d["x_next"].tolist() == [0.5, 0.0] and d["dual_slack"].tolist() == [-2.0, 4.0] and d["x_reflected"].tolist() == [-1.0, -2.0]
    assert d["y_next"].tolist() == [4.0, -6.0] and d["y_reflected"].tolist() == [4.0, -8.0]
    assert d["x"].tolist() == [1.0, 2.0] and d["y"].tolist() == [3.0, -5.0]


def test_halpern_step_by_hand_free_branches_minor_step_and_weight():
    """The same problem from x = (5/4, 4): temp = (1/4, 1), both inside: proj = temp, slack = 0, x_reflected = (-3/4, -2);
    A x_reflected = (-19/4, -41/4); temp_y = (27/4, 33/4).  Row 0: [-inf, 8] and row 1: [8, 20]: both inside, dual = 0,
    y_reflected = -y = (-4, 4).  hIter = 2, k = 1: w = 3/4; x = 3/4 (-3/4, -2) + 1/4 (3, 6) = (3/16, 0);
    y = 3/4 (-4, 4) + 1/4 (2, -2) = (-5/2, 5/2).  A minor step leaves x_next, y_next and dual_slack alone."""
    A, d = _hand([1.25, 4.0], [-8.0, -20.0], [INF, -8.0])
    keep = dict(x_next=np.array([7.0, 7.0]), y_next=np.array([8.0, 8.0]), dual_slack=np.array([9.0, 9.0]))
    d.update({k: a.copy() for k, a in keep.items()})
    temp = H.halpern_step(A, d, 0.25, 2.0, 2, 1, False)
    assert temp.tolist() == [0.25, 1.0]
    for k, a in keep.items():
        assert np.array_equal(d[k], a), k
    assert d["x_reflected"].tolist() == [-0.75, -2.0] and d["y_reflected"].tolist() == [-4.0, 4.0]
    assert d["x"].tolist() == [0.1875, 0.0] and d["y"].tolist() == [-2.5, 2.5]
    A, d = _hand([1.25, 4.0], [-8.0, -20.0], [INF, -8.0])
    H.halpern_step(A, d, 0.25, 2.0, 2, 1, True)
    assert d["x_next"].tolist() == [0.25, 1.0] and d["dual_slack"].tolist() == [0.0, 0.0] and d["y_next"].tolist() == [0.0, 0.0]


def test_halpern_step_by_hand_on_the_bounds():
    """x = (3/2, 3): temp = (1/2, 0): column 0 exactly on u, column 1 exactly on l: proj = (1/2, 0), slack = 0,
    x_reflected = (-1/2, -3); A x_reflected = (-13/2, -27/2); temp_y = (17/2, 23/2).  Row 0 an equality at rl = ru = -17/2:
    dual = 0.  Row 1 ranged [rl, ru] = [-12, -23/2]: temp_y sits on -ru: dual = 0."""
    A, d = _hand([1.5, 3.0], [-8.5, -12.0], [-8.5, -11.5])
    temp = H.halpern_step(A, d, 0.25, 2.0, 0, 1, True)
    assert temp.tolist() == [0.5, 0.0] and d["x_next"].tolist() == [0.5, 0.0] and d["dual_slack"].tolist() == [0.0, 0.0]
    assert d["x_reflected"].tolist() == [-0.5, -3.0] and d["y_next"].tolist() == [0.0, 0.0] and d["y_reflected"].tolist() == [-4.0, 4.0]
