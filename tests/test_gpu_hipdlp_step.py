"""The Halpern step of solver="hipdlp" (hipdlp/pdhg.cc:961-1018 of the reference implementation) on the problems that sit on
the structural thresholds of the SpMV launches — the long-major limits 256 / 512 / 2048, contained and spanning segment tasks,
idle-task padding, the 512 -> 1024 segment length, work blocks capped at 2048 majors, work blocks without entries, more than
2048 long majors, grids of 32 / 33 and 64 / 65 workgroups — in every launch form that runs it:
  plain, stream layout   Epi<kHalpernPrimal> / Epi<kHalpernDual> of k_spmv and, for long majors, of longBlock
  plain, slab layout     the same epilogues in k_spmv_slab and in the slab layout's segment tasks
  persistent             halpernSmallPass of pdlp_halpern_small.hip, XCD-local and agent scope
Cases, planted starts and the numbers every case must show: tests/hipdlp_step_cases.py; what they rely on is proven without a
GPU in tests/test_hipdlp_step_host.py.  The reference is hipdlp_check_cases.halpern_step, an elementwise restatement that knows
nothing of blocks, lanes or segments.

  a. integer matrix, planted dyadic start: every product of the step is exact in ANY summation order, so x, x_next,
     x_reflected, dual_slack, y, y_next, y_reflected must `==` the restatement — one step with a real dual step size and real
     anchors, two steps on a dyadic grid — with every marked major (long, first or last of a work block, in a block without
     entries) strictly inside its bounds in one plan and on or beyond a bound in the other;
  b. the same two steps with the second one inside the persistent launch, at 4, 8, 11, 32, 33 and 64 workgroups;
  c. real data, 40 steps: the plain launches and the persistent launch leave the same bits in all nine iterate vectors;
  d. real data, one step: x_next and y_next within a derived bound that holds for any summation order.
Every test asserts the instantiation it claims to run: the layout and the plan numbers from what the device holds
(DeviceSolver.device_matrix), the reason and mode of the persistent rule, the launch count, no fall-back."""
import numpy as np
import pytest

import edge_cases as E
import hipdlp_check_cases as H
import hipdlp_step_cases as SC
from highs_amd import solver

pytestmark = pytest.mark.gpu

NAN_VECTORS = ("x_next", "y_next", "x_reflected", "y_reflected", "dual_slack")
STEP_DATA = ("x", "y", "x_anchor", "y_anchor", "lower", "upper", "cost", "rhs", "row_upper")
_open = {}


@pytest.fixture(scope="module", autouse=True)
def _close_the_kept_solver():
    """(the integer tests keep one solver open between them: the last one is closed behind the module)"""
    yield
    for k in list(_open):
        _open.pop(k).close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _nan_pattern(k, tag):
    return (np.uint64(0x7FF8000000000000) + np.uint64(tag << 32) + np.arange(1, k + 1, dtype=np.uint64)).view(np.float64)


def _len(S, name):
    return S.m if name in H.ROW_VECTORS or name == "row_upper" else S.n


def _get(S, name):
    return S.get(name, _len(S, name))


def _stage(S, name):
    return int(S.stage(name)[0])


def _assert_layout(S, name, layout):
    """What the device built of both operands is what the case claims (hipdlp_step_cases.EXPECT, proven on the host planners)."""
    ex, plans = SC.EXPECT[name], SC.plans(name)
    for which, stream, slab_long, group in ((0, ex.a, ex.slab[0], ex.group), (1, ex.at, ex.slab[1], 1)):
        D = S.device_matrix(which)
        print(name, layout, "operand", which, {k: D[k] for k in ("use_slab", "chunk", "n_blocks", "n_long", "n_tasks", "task_group", "long_group", "long_slots", "slab_blocks")})
        if layout == "csr":
            assert (D["use_slab"], D["chunk"], D["n_blocks"], D["n_long"], D["n_tasks"], D["long_group"]) == (0, ex.chunk) + stream + (1,)
            assert np.array_equal(D["block_beg"], plans[which]["blocks"])
        else:  # every major beyond 256 entries is segment tasks (their deal follows the device's CU count), no stream block
            assert (D["use_slab"], D["n_blocks"], D["n_long"], D["long_group"]) == (1, 0, slab_long, group)
            assert np.array_equal(D["long_map"], plans[2 + which]["long_majors"])
            T = D["tasks"]
            assert D["n_tasks"] >= slab_long and (D["n_tasks"] == 0) == (slab_long == 0)
            assert sorted(set(T[T[:, 2] >= 0, 2].tolist())) == list(range(slab_long))  # every long major has its tasks


def _create(name, layout, values, persistent, monkeypatch, xcd_local=None, **options):
    for k in list(_open):  # (never two solvers of this module at once)
        _open.pop(k).close()
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1" if layout == "slab" else "0")
    monkeypatch.setenv("PDLP_MI355X_PERSISTENT_HIPDLP", "1" if persistent else "0")
    if xcd_local is not None:
        monkeypatch.setenv("PDLP_MI355X_XCD_LOCAL", xcd_local)
    S = solver.DeviceSolver(lp=SC.case_lp(name, values), solver="hipdlp", **options)
    lp = SC.case_lp(name, values)
    assert (S.n, S.m, S.n_eqs) == (lp.num_col, lp.num_row, 0)
    return S


def _integer_solver(name, layout, persistent, monkeypatch, xcd_local=None):
    """One solver per (case, layout, form), kept for the tests that follow one another on it; the one before is closed."""
    key = (name, layout, persistent, xcd_local)
    if key not in _open:
        S = _create(name, layout, "integer", persistent, monkeypatch, xcd_local, pdlp_features_off=1)
        assert S.setup_scalars()["scaled"] == 0.0
        _assert_layout(S, name, layout)
        _open[key] = S
    return _open[key]


def _run_steps(S, d, stage, k, sigma, h_iter):
    """Plants the start d and NaN patterns in everything a major step writes, runs `stage` with k steps: -> the seven vectors."""
    for key in STEP_DATA:
        S.set(key, d[key])
    for key in NAN_VECTORS:
        S.set(key, _nan_pattern(_len(S, key), 5))
    S.set("halpern_state", H.state_array(dict(H.BASE, tau=SC.TAU, sigma=sigma, hIter=h_iter), False))
    S.stage(stage, 16, init=[k])
    for key in STEP_DATA[2:]:  # a step changes no datum
        assert np.array_equal(_bits(_get(S, key)), _bits(d[key])), key
    return {key: _get(S, key) for key in H.STEP_VECTORS}


def _assert_equals_restatement(name, plan_name, got, d, k, sigma, h_iter, what):
    want, trace = SC.restate(name, d, k, sigma, h_iter)
    F = SC.formulated(name)
    A, At = F.A.tocsr(), F.A.T.tocsr()
    for tr in trace:  # the premise: both products of every step are exact in any order
        assert SC.exact_units(At, tr["aty_operand"])[1] < 2.0**53 and SC.exact_units(A, tr["ax_operand"])[1] < 2.0**53
    rows, cols = SC.marked(name)
    cc, rc = trace[0]["col_class"][cols], trace[0]["row_class"][rows]
    if plan_name == "free":
        assert np.all(cc == 0) and np.all(rc == 0)
    else:
        assert np.all(cc != 0) and np.all(rc != 0) and (np.abs(cc) == 2).any() and (np.abs(rc) == 2).any()
    if k == 2:  # the second step (the persistent launch's, in b) is not planned, but some marked major carries its sum there too:
        assert (trace[1]["col_class"][cols] == 0).any() and (trace[1]["row_class"][rows] != 0).any()  # an unclamped column, a clamped row
    for key in H.STEP_VECTORS:
        bad = np.nonzero(got[key] != want[key])[0]
        assert bad.size == 0, (what, key, bad[:8], got[key][bad[:4]], want[key][bad[:4]])
    # x_next is a selection between temp, l and u: the bits of the selected one, the sign of a zero included (-0.0 bounds)
    assert np.array_equal(_bits(got["x_next"]), _bits(want["x_next"])), (what, "x_next bits", np.nonzero(_bits(got["x_next"]) != _bits(want["x_next"]))[0][:8])


SETTINGS = {1: (0.37, 7, False), 2: (2.0, 0, True)}  # k -> (sigma, hIter, dyadic anchors)


# ---- a: the plain launches, both layouts ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("plan_name", SC.PLANS)
@pytest.mark.parametrize("name,layout", SC.PARAMS)
def test_integer_step_is_exact(name, layout, plan_name, k, monkeypatch):
    """stage steps, k = 1: one major step with tau = 1/4, sigma = 0.37, hIter = 7 (w = 8 / 9) and real anchors; k = 2: two major
    steps with sigma = 2, hIter = 0 (w = 1 / 2, then 2 / 3) and dyadic anchors, so that the second step's products are exact
    too.  All seven vectors == the restatement."""
    S = _integer_solver(name, layout, False, monkeypatch)
    assert _stage(S, "persistent_reason") != 0 and _stage(S, "persistent_mode") == -1
    sigma, h_iter, dyadic = SETTINGS[k]
    d = SC.step_data(name, plan_name, np.random.default_rng(23), sigma=sigma, dyadic_anchors=dyadic)
    got = _run_steps(S, d, "steps", k, sigma, h_iter)
    assert _stage(S, "persistent_launches") == 0 and _stage(S, "barrier_fallbacks") == 0
    _assert_equals_restatement(name, plan_name, got, d, k, sigma, h_iter, (name, layout, plan_name, k))


# ---- b: the second step inside the persistent launch ---------------------------------------------------------------------------
PERSISTENT_PARAMS = [(n, None) for n in SC.PERSISTENT_CASES] + [("empty_runs", "0"), ("grid32", "0")]


@pytest.mark.parametrize("name,xcd_local", PERSISTENT_PARAMS, ids=["%s-%s" % (n, "default" if x is None else "agent") for n, x in PERSISTENT_PARAMS])
def test_integer_step_through_the_persistent_launch(name, xcd_local, monkeypatch):
    """stage steps_persistent with k = 2 (step 1 by the plain launches, step 2 — the major one — as ONE persistent launch), both
    plans, == the restatement.  `agent`: PDLP_MI355X_XCD_LOCAL=0, agent-scope accesses below 33 workgroups too."""
    S = _integer_solver(name, "csr", True, monkeypatch, xcd_local)
    reason, grid, mode = SC.EXPECT[name].rule
    mode = 0 if xcd_local == "0" else mode
    sigma, h_iter, dyadic = SETTINGS[2]
    for plan_name in SC.PLANS:
        assert _stage(S, "persistent_reason") == 0 and _stage(S, "persistent_mode") == mode
        before = _stage(S, "persistent_launches")
        d = SC.step_data(name, plan_name, np.random.default_rng(23), sigma=sigma, dyadic_anchors=dyadic)
        got = _run_steps(S, d, "steps_persistent", 2, sigma, h_iter)
        assert _stage(S, "persistent_launches") == before + 1 and _stage(S, "barrier_fallbacks") == 0
        assert _stage(S, "persistent_reason") == 0 and _stage(S, "persistent_mode") == mode
        _assert_equals_restatement(name, plan_name, got, d, 2, sigma, h_iter, (name, xcd_local, plan_name))


def test_65_work_blocks_keep_the_plain_launches(monkeypatch):
    S = _integer_solver("grid65", "csr", True, monkeypatch)
    assert _stage(S, "persistent_reason") == 7 and _stage(S, "persistent_mode") == -1
    with pytest.raises(RuntimeError, match="keeps the plain launches"):
        S.stage("steps_persistent", 16, init=[2])
    assert _stage(S, "persistent_launches") == 0


# ---- c: the forms over a block --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SC.PERSISTENT_CASES)
def test_forms_agree_over_a_block(name, monkeypatch):
    """Real data, default options (scaling on), 40 steps from one planted start: as plain launches (switch off) and as step 1 +
    ONE persistent launch of the steps 2..40 (switch on), all nine iterate vectors bit for bit.  This is what reaches the MINOR
    steps inside the persistent launch (h.major == 0: x_next, y_next, dual_slack and y_reflected are left alone until step 40).
    An exact three-step case does not exist: the blends k / (k + 1) of two consecutive steps are never both dyadic, so behind
    the second blend the operands leave every dyadic grid and a third step's products depend on their summation order."""
    rng = np.random.default_rng(31)
    lp = SC.case_lp(name, "real")
    start = dict(x=rng.uniform(-0.5, 1.5, lp.num_col), y=rng.standard_normal(lp.num_row), x_anchor=rng.uniform(0.0, 1.0, lp.num_col),
                 y_anchor=rng.standard_normal(lp.num_row))
    reason, grid, mode = SC.EXPECT[name].rule
    out = {}
    for persistent in (False, True):
        S = _create(name, "csr", "real", persistent, monkeypatch)
        assert S.setup_scalars()["scaled"] == 1.0
        for which, stream in ((0, SC.EXPECT[name].a), (1, SC.EXPECT[name].at)):
            D = S.device_matrix(which)
            assert (D["use_slab"], D["n_blocks"], D["n_long"], D["n_tasks"]) == (0,) + stream
        assert (_stage(S, "persistent_reason") == 0) == persistent and _stage(S, "persistent_mode") == (mode if persistent else -1)
        for key, a in start.items():
            S.set(key, a)
        for key in NAN_VECTORS:
            S.set(key, _nan_pattern(_len(S, key), 6))
        S.set("halpern_state", H.state_array(dict(H.BASE, hIter=0), True))
        S.stage("steps_persistent" if persistent else "steps", 16, init=[40])
        assert _stage(S, "persistent_launches") == (1 if persistent else 0) and _stage(S, "barrier_fallbacks") == 0
        assert (_stage(S, "persistent_reason") == 0) == persistent and _stage(S, "persistent_mode") == (mode if persistent else -1)
        out[persistent] = {key: _get(S, key) for key in H.ITERATE}
        S.close()
    for key in H.ITERATE:
        assert not np.isnan(out[False][key]).any(), key
        assert np.array_equal(_bits(out[False][key]), _bits(out[True][key])), (name, key, np.nonzero(_bits(out[False][key]) != _bits(out[True][key]))[0][:8])
    assert not np.array_equal(out[False]["x"], start["x"]) and not np.array_equal(out[False]["y"], start["y"])


# ---- d: real data within the any-order bound ------------------------------------------------------------------------------------
REAL_PARAMS = [(n, l) for n in ("limit512", "limit2048", "segments", "empty_runs4600") for l in ("csr", "slab")] + [("long2049", "slab")]


@pytest.mark.parametrize("name,layout", REAL_PARAMS)
def test_real_step_within_the_any_order_bound(name, layout, monkeypatch):
    """Real matrix data without scaling, one major step with tau = 2^-2, sigma = 2, hIter = 7, the problem's own cost and column
    bounds ([0, 1]), rows with rl finite and ru = inf, a real start that leaves every marked major (long, first or last of a
    work block, in a block without entries) and every second other one UNCLAMPED on the column side and CLAMPED on the row
    side — where x_next = temp and y_next = sigma (temp_y + rl) carry the product; a projected-away product would be judged
    on a constant.  Nothing is measured; with u = 2^-53, k_j the entries of
    major j, s' the exactly rounded product (edge_cases.exact_major_sums) and s the device's:
      |s - s'| <= delta_j = (k_j + 1) u sum|a_i v_i|     (any order: gamma_k sum|a_i v_i|, Higham 4.2; the reference's own
                                                         rounding u |s'|; the factor 1 / (1 - k u) is in the 1 + 1e-6 below)
    Column side, operand the planted y.  Device and reference both compute q = fl(c - s), then temp = fl(x - tau q), tau q exact
    (a power of two):  |q - q'| <= delta + u |c - s| + u |c - s'| <= delta + 2u (|c| + |s'|) to first order;
    |temp - temp'| <= tau |q - q'| + u |temp| + u |temp'| <= tau delta + 2u tau (|c| + |s'|) + 2u (|x| + tau (|c| + |s'|)).
    x_next = proj(temp) is a selection, and the projection is 1-Lipschitz:
      |x_next - proj(temp')| <= (tau delta + 2u |x| + 4u tau (|c| + |s'|)) (1 + 1e-6).
    Row side, operand the DEVICE'S x_reflected, so that this product is judged on what the device gathered.  y / sigma is exact;
    temp_y = fl(y / 2 - s): |temp_y - temp_y'| <= delta + 2u |temp_y'|; g(t) = t - clamp(t) is 1-Lipschitz and its subtraction
    rounds once on either side, the multiplication by sigma = 2 is exact:
      |y_next - pd'| <= sigma (delta + 2u |temp_y'| + 2u |temp_y' - proj_y'|) (1 + 1e-6).
    dual_slack = (x_next - temp) / tau needs the device's temp, which no hook returns: asserted is its sign against the clamp
    class, wherever the class is the same at temp' - bound and temp' + bound; and x_next inside its bounds."""
    lp = SC.case_lp(name, "real")
    F = H.formulated_lp(lp, "integer")  # (the options of the integer cases: no scaling; the data are the real LP's)
    FI = SC.formulated(name)
    assert np.array_equal(F.A.indptr, FI.A.indptr) and np.array_equal(F.A.indices, FI.A.indices)  # the integer case's pattern
    assert np.all(F.col_scale == 1.0) and np.all(F.row_scale == 1.0) and not np.array_equal(F.A.data, np.rint(F.A.data))
    S = _create(name, layout, "real", False, monkeypatch, pdlp_features_off=1)
    assert S.setup_scalars()["scaled"] == 0.0 and _stage(S, "persistent_reason") != 0
    ex = SC.EXPECT[name]
    for which, stream, slab_long, group in ((0, ex.a, ex.slab[0], ex.group), (1, ex.at, ex.slab[1], 1)):
        D = S.device_matrix(which)
        if layout == "csr":
            assert (D["use_slab"], D["n_blocks"], D["n_long"], D["n_tasks"], D["long_group"]) == (0,) + stream + (1,)
        else:
            assert (D["use_slab"], D["n_blocks"], D["n_long"], D["long_group"]) == (1, 0, slab_long, group)
    cost, lower, upper, rl0, ru = (_get(S, k) for k in ("cost", "lower", "upper", "rhs", "row_upper"))
    assert np.array_equal(cost, F.cost) and np.array_equal(lower, F.lower) and np.array_equal(upper, F.upper)
    assert np.array_equal(rl0, F.rhs) and np.array_equal(ru, F.row_upper) and np.all(ru == H.INF)
    assert np.all(lower == 0.0) and np.all(upper == 1.0)
    csc, csr = F.A.tocsc(), F.A.tocsr()
    csc.sort_indices(); csr.sort_indices()
    rng = np.random.default_rng(37)
    tau, sigma, h_iter, u = 0.25, 2.0, 7, 2.0**-53
    mark_rows, mark_cols = SC.marked(name)
    show_cols, show_rows = mark_cols | (np.arange(F.n) % 2 == 0), mark_rows | (np.arange(F.m) % 2 == 0)
    d = dict(y=rng.standard_normal(F.m), x_anchor=rng.standard_normal(F.n), y_anchor=rng.standard_normal(F.m))
    # column side: the start puts temp of every marked and every second column strictly inside [0, 1], the others anywhere
    s1, scale1, lens1 = E.exact_major_sums(csc.indptr, csc.indices, csc.data, d["y"])
    d["x"] = tau * (cost - s1) + np.where(show_cols, rng.uniform(0.2, 0.8, F.n), rng.uniform(-1.0, 2.0, F.n))

    def step(rl):
        for key, a in d.items():
            S.set(key, a)
        S.set("rhs", rl)
        for key in NAN_VECTORS:
            S.set(key, _nan_pattern(_len(S, key), 7))
        S.set("halpern_state", H.state_array(dict(H.BASE, tau=tau, sigma=sigma, hIter=h_iter), False))
        S.stage("steps", 16, init=[1])
        assert _stage(S, "persistent_launches") == 0
        return {key: _get(S, key) for key in H.STEP_VECTORS}

    first = step(rl0)
    # row side: no row bound enters x_reflected, so a second run of the same start gathers the same bits; its row bounds put
    # every marked and every second row BEYOND -rl (y_next = 2 (temp_y + rl) carries the product), the others inside (y_next = 0)
    s2, scale2, lens2 = E.exact_major_sums(csr.indptr, csr.indices, csr.data, first["x_reflected"])
    temp_y = d["y"] / sigma - s2
    rl = -temp_y + np.where(show_rows, 1.0, -1.0) * rng.uniform(0.5, 1.5, F.m)
    got = step(rl)
    S.close()
    assert np.array_equal(_bits(got["x_reflected"]), _bits(first["x_reflected"])) and np.array_equal(_bits(got["x_next"]), _bits(first["x_next"]))
    # column side
    delta = (lens1 + 1) * u * scale1
    temp1 = d["x"] - tau * (cost - s1)
    bound = (tau * delta + 2 * u * np.abs(d["x"]) + 4 * u * tau * (np.abs(cost) + np.abs(s1))) * (1 + 1e-6)
    err = np.abs(got["x_next"] - H._std_max(lower, H._std_min(temp1, upper)))
    w = int(np.argmax(err / bound))
    print(name, layout, "x_next worst column", w, "entries", lens1[w], "error", err[w], "bound", bound[w], "ratio", err[w] / bound[w])
    assert np.all(err <= bound), np.nonzero(err > bound)[0][:8]
    assert np.all(got["x_next"] >= lower) and np.all(got["x_next"] <= upper)
    assert np.all((got["x_next"][show_cols] > 0.0) & (got["x_next"][show_cols] < 1.0))  # (x_next IS temp there: the product shows)
    assert np.array_equal(got["x_reflected"], 2.0 * got["x_next"] - d["x"])  # (elementwise on the device's own x_next)
    below, above = temp1 + bound < lower, temp1 - bound > upper
    inside = (temp1 - bound > lower) & (temp1 + bound < upper)
    assert below.any() and above.any() and inside[show_cols].all()
    assert np.all(got["dual_slack"][below] > 0) and np.all(got["dual_slack"][above] < 0) and np.all(got["dual_slack"][inside] == 0)
    # row side, on the device's own x_reflected
    delta = (lens2 + 1) * u * scale2
    proj_y = H._std_max(-ru, H._std_min(temp_y, -rl))
    pd = (temp_y - proj_y) * sigma
    bound = sigma * (delta + 2 * u * np.abs(temp_y) + 2 * u * np.abs(temp_y - proj_y)) * (1 + 1e-6)
    err = np.abs(got["y_next"] - pd)
    w = int(np.argmax(err / bound))
    print(name, layout, "y_next worst row", w, "entries", lens2[w], "error", err[w], "bound", bound[w], "ratio", err[w] / bound[w])
    assert np.all(err <= bound), np.nonzero(err > bound)[0][:8]
    assert np.all(got["y_next"][show_rows] > 0.9) and np.all(got["y_next"][~show_rows] == 0.0)
    assert np.array_equal(got["y_reflected"], 2.0 * got["y_next"] - d["y"])
    k = h_iter + 1
    wgt = float(k) / (k + 1.0)
    assert np.array_equal(got["x"], wgt * got["x_reflected"] + (1.0 - wgt) * d["x_anchor"])
    assert np.array_equal(got["y"], wgt * got["y_reflected"] + (1.0 - wgt) * d["y_anchor"])
