"""The 30 sums of a check iteration (tests/check_cases.py has their definitions) and the 20 numbers derived from them, in all
three forms that compute them, against references that depend on no summation order:

  form "one"   the one-launch check of the persistent small loop (pdlp_check.hip checkSmallBody; k_check_small_qp for a QP
               with off-diagonal Hessian entries)                          stage check_device, check_launches == 1
  form "seq"   the device-driven launch sequence (k_row_stats2 / k_col_stats2 / k_final_reduce2 behind the gate)
                                                                           stage check_device, check_launches == 10
  form "host"  the same kernels called from Solver::computeResiduals      stage residuals
Every case asserts the form it runs through check_launches: "seq" is forced with PDLP_MI355X_CHECK_SMALL=0 where the loop would
take the problem, and asserted WITHOUT the switch where it does not (so the case also shows that the loop declines it).

  a. integer data, no scaling (pdlp_features_off = 1), fresh solver (sumPrimalStep == 0: x_avg = x_sum exactly): every sum is
     an integer (1/2 x'Qx: a half-integer) below 2^53 in any order — `==` with the int64 value; the four slack vectors `==`.
  b. real data, scaling on: |gpu - fsum| <= (len + 1) 2^-53 sum|term| (1 + 1e-6) per quantity — the bound for ANY summation
     order that tests/test_gpu_edges.py derives (the terms themselves carry the same roundings on both sides: no contraction,
     IEEE division); also behind 40 and 80 iterations of a default solver (sumPrimalStep > 0, a pending average weight).
  c. the 30 sums and the 20 derived numbers of the three forms on the same planted state: bit-identical ("the same tree").
  d. the 20 derived numbers `==` check_cases.derived of the 30 sums, in every case above and on a cold start (both norms fall
     back to 1) and a state with a negative ray objective.
  e. a and b on QPs (diagonal; with off-diagonal entries), and b on a small QP of tests/qp_small_cases.py (its real Hessian
     cannot be replaced by integers on the device, so a has no such case).

Sizes (check_cases.SIZES): one element; 255 x 257; 256 x 256; 65537 columns (257 blocks; the thin variant is the one the
one-launch check takes: 257 virtual blocks on 64 workgroups); 196608 x 196609 (768 / 769 partials: the unrolled loop of the
final reduction starts at 769); 524288 x 524289 (the last size without the grid-stride loop of the statistics kernels and
the first with it).  The one-launch form also runs on the grid 32 / 33 / 64 cases and wide(16385) of tests/edge_cases.py with
planted data (grid65 has 65 workgroups: the loop hands its checks to the launch sequence, which is what is asserted there)."""
import numpy as np
import pytest

import check_cases as K
import edge_cases as E
import qp_small_cases as Q
from highs_amd import solver

pytestmark = pytest.mark.gpu

SWITCH = "PDLP_MI355X_CHECK_SMALL"
# case -> (maker(values, qp), forms, plant the data too)
ALL, NO_LOOP = ("one", "seq", "host"), ("seq", "host")
CASES = {
    "1x1": (lambda v, qp: K.sized_lp(1, 1, v, qp), ALL, False),
    "255x257": (lambda v, qp: K.sized_lp(255, 257, v, qp), ALL, False),
    "256x256": (lambda v, qp: K.sized_lp(256, 256, v, qp), ALL, False),
    "65537x300": (lambda v, qp: K.sized_lp(65537, 300, v, qp), NO_LOOP, False),
    "65537x300thin": (lambda v, qp: K.sized_lp(65537, 300, v, qp, thin=True), ALL, False),
    "196608x196609": (lambda v, qp: K.sized_lp(196608, 196609, v, qp), NO_LOOP, False),
    "524288x524289": (lambda v, qp: K.sized_lp(524288, 524289, v, qp), NO_LOOP, False),
    "grid32": (lambda v, qp: E.grid(32, v), ("one",), True),
    "grid33": (lambda v, qp: E.grid(33, v), ("one",), True),
    "grid64": (lambda v, qp: E.grid(64, v), ("one",), True),
    "grid65": (lambda v, qp: E.grid(65, v), ("seq",), True),
    "wide16385": (lambda v, qp: E.wide(16385, v), ("one",), True),
}
LP_PARAMS = [(c, f) for c, (_, forms, _) in CASES.items() for f in forms]
QP_PARAMS = [(c, qp, f) for c in ("255x257", "65537x300") for qp in ("diag", "sparse") for f in CASES[c][1]]
_made, _runs = {}, {}


def _lp(case, values, qp=None):
    key = (case, values, qp)
    if key not in _made:
        _made[key] = CASES[case][0](values, qp)
    return _made[key]


def _options(values):
    return dict(pdlp_features_off=1) if values == "integer" else {}


def _create(lp, form, loop_takes_it, monkeypatch, **options):
    """A solver whose device-driven check has the form asked for — asserted, never assumed."""
    monkeypatch.delenv(SWITCH, raising=False)
    if form == "seq" and loop_takes_it:
        monkeypatch.setenv(SWITCH, "0")
    S = solver.DeviceSolver(lp, **options)
    launches, one = int(S.stage("check_launches", 1)[0]), int(S.stage("small_loop", 3)[2])
    if form == "one" or (form == "host" and loop_takes_it):
        assert (launches, one) == (1, 1), (lp.model_name, form, launches, one)
    else:
        assert (launches, one) == (10, 0), (lp.model_name, form, launches, one)
    return S


def _check(S, form):
    """One check of the present state in the form `form`; the 50 numbers of check_stats."""
    if form == "host":
        S.stage("residuals")
    else:
        assert S.stage("check_device", 1)[0] == 1.0  # the record's `ran`
    return S.stage("check_stats", 50)


def _run(case, values, qp, form, monkeypatch):
    """The case in one form, on the state planted with the case's seed: run once, kept.  The first form's read-back gives the
    reference; every later form must hold the same vectors (then the reference is shared, unchanged)."""
    key = (case, values, qp)
    kept = _runs.setdefault(key, {"forms": {}})
    if form in kept["forms"]:
        return kept
    lp = _lp(case, values, qp)
    S = _create(lp, form, "one" in CASES[case][1], monkeypatch, **_options(values))
    scaled = values != "integer"
    assert S.get("steps", 8)[6] == 0.0  # sumPrimalStep: the averages are the running sums themselves
    K.plant(S, values, np.random.default_rng(11), data=CASES[case][2])
    out = _check(S, form)
    v = K.read_vectors(S, scaled)
    slacks = {k: S.get(k, S.n) for k in ("slack_pos", "slack_neg", "slack_pos_avg", "slack_neg_avg")}
    n_eqs = S.n_eqs
    assert np.array_equal(v["x_avg"], S.get("x_sum", S.n)) and np.array_equal(v["y_avg"], S.get("y_sum", S.m))
    if qp == "sparse":
        assert "nx" in v and "qdiag" in v
    assert (qp is not None) == ("qdiag" in v)
    S.close()
    if "vectors" not in kept:
        kept["vectors"] = v
        kept["ref"] = K.reference_stats(v, n_eqs, scaled, lp.sense, lp.offset, integer=(values == "integer"))
    else:
        assert sorted(v) == sorted(kept["vectors"])
        for k in v:
            assert np.array_equal(v[k], kept["vectors"][k]), (case, form, k)
    kept["forms"][form] = (out, slacks)
    return kept


def _assert_slacks(kept, form, what):
    for k, got in kept["forms"][form][1].items():
        assert np.array_equal(got, kept["ref"][k]), (what, form, k, np.nonzero(got != kept["ref"][k])[0][:8])


def _assert_derived(out, ref, what):
    want = K.derived(out[:30], ref["qp"], ref["sense"], ref["offset"])
    assert np.array_equal(out[30:50], want), (what, [(K.DERIVED_NAMES[k % 10], out[30 + k], want[k]) for k in np.nonzero(out[30:50] != want)[0]])


def _assert_exact(kept, form, what):
    out, ref = kept["forms"][form][0], kept["ref"]
    assert all(q.abs_sum < 2.0**53 for q in ref["q"])
    want = K.exact_values(ref)
    bad = np.nonzero(out[:30] != want)[0]
    assert bad.size == 0, (what, form, [(K.NAMES[k], out[k], want[k]) for k in bad])
    _assert_slacks(kept, form, what)
    _assert_derived(out, ref, what)


def _assert_within_bound(kept, form, what):
    out, ref = kept["forms"][form][0], kept["ref"]
    err = np.array([abs(out[k] - q.fsum) for k, q in enumerate(ref["q"])])
    bound = np.array([K.any_order_bound(q) for q in ref["q"]])
    worst = int(np.argmax(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), np.where(err > 0, np.inf, 0.0))))
    print(what, form, "worst quantity", K.NAMES[worst], "length", ref["q"][worst].length, "error", err[worst], "bound", bound[worst])
    assert np.all(err <= bound), (what, form, [(K.NAMES[k], out[k], ref["q"][k].fsum, err[k], bound[k]) for k in np.nonzero(err > bound)[0]])
    _assert_slacks(kept, form, what)
    _assert_derived(out, ref, what)


# ---- a, b: every form at every size ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", LP_PARAMS)
def test_integer_data_gives_the_exact_sums(case, form, monkeypatch):
    _assert_exact(_run(case, "integer", None, form, monkeypatch), form, case)


@pytest.mark.parametrize("case,form", LP_PARAMS)
def test_real_data_stays_within_the_any_order_bound(case, form, monkeypatch):
    _assert_within_bound(_run(case, "real", None, form, monkeypatch), form, case)


# ---- e: QPs -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,qp,form", QP_PARAMS)
def test_qp_integer_data_gives_the_exact_sums(case, qp, form, monkeypatch):
    kept = _run(case, "integer", qp, form, monkeypatch)
    _assert_exact(kept, form, case + qp)
    half = kept["ref"]["q"][8 + K.COL_STATS - 1]
    assert half.abs_sum > 0 and (qp == "diag" or np.any(half.terms != np.rint(half.terms)))  # half-integers, exact


@pytest.mark.parametrize("case,qp,form", QP_PARAMS)
def test_qp_real_data_stays_within_the_any_order_bound(case, qp, form, monkeypatch):
    _assert_within_bound(_run(case, "real", qp, form, monkeypatch), form, case + qp)


def test_small_qp_on_the_one_launch_qp_check(monkeypatch):
    """portfolio(64): a dense Hessian, the persistent QP loop with its own one-launch check (k_check_small_qp)."""
    monkeypatch.delenv(SWITCH, raising=False)
    lp = Q.portfolio()
    S = solver.DeviceSolver(lp)
    assert int(S.stage("check_launches", 1)[0]) == 1 and int(S.stage("trial_barriers", 1)[0]) == 3  # (three barriers: the QP loop)
    K.plant(S, "real", np.random.default_rng(12), data=True)
    assert S.stage("check_device", 1)[0] == 1.0
    out = S.stage("check_stats", 50)
    v = K.read_vectors(S, True)
    assert "nx" in v and "nx_avg" in v and "qdiag" in v
    kept = {"ref": K.reference_stats(v, S.n_eqs, True, lp.sense, lp.offset),
            "forms": {"one": (out, {k: S.get(k, S.n) for k in ("slack_pos", "slack_neg", "slack_pos_avg", "slack_neg_avg")})}}
    S.close()
    _assert_within_bound(kept, "one", lp.model_name)


# ---- b: behind 40 and 80 iterations ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", [("255x257", "one"), ("255x257", "seq"), ("65537x300thin", "one"), ("65537x300", "seq")])
def test_check_behind_a_running_solve(case, form, monkeypatch):
    """A default solver (restarts on) stopped at a check iteration: the running sums carry weights, a pending average weight
    exists.  The state is read first, then the check runs; it must leave the iterate alone (check_device: restarts off)."""
    lp = _lp(case, "real")
    S = _create(lp, form, "one" in CASES[case][1], monkeypatch)
    for _ in (40, 80):
        st = S.iterate(40)
        assert st.iters == 40
        steps = S.get("steps", 8)
        print(case, form, "sumPrimalStep", steps[6], "pending average weight", steps[7])
        assert steps[6] > 0.0 and steps[7] >= 0.0
        before = {k: S.get(k, S.m if k in ("y", "ax") else S.n) for k in ("x", "y", "ax", "aty")}
        assert S.stage("check_device", 1)[0] == 1.0
        out = S.stage("check_stats", 50)
        v = K.read_vectors(S, True)
        for k in before:
            assert np.array_equal(before[k], v[k]), k
        assert S.get("steps", 8)[7] == 0.0  # the check has flushed the pending weight
        kept = {"ref": K.reference_stats(v, S.n_eqs, True, lp.sense, lp.offset),
                "forms": {form: (out, {k: S.get(k, S.n) for k in ("slack_pos", "slack_neg", "slack_pos_avg", "slack_neg_avg")})}}
        _assert_within_bound(kept, form, case)
    with pytest.raises(RuntimeError, match="not a check iteration"):  # never forced
        S.iterate(1)
        S.stage("check_device", 1)
    S.close()


# ---- c: the three forms agree bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("case,values,qp", [("255x257", "real", None), ("65537x300thin", "real", None), ("65537x300thin", "integer", None),
                                            ("255x257", "real", "sparse"), ("255x257", "real", "diag"), ("1x1", "real", None),
                                            ("196608x196609", "real", None), ("524288x524289", "real", None)])
def test_forms_agree_bit_for_bit(case, values, qp, monkeypatch):
    forms = CASES[case][1]
    for form in forms:
        kept = _run(case, values, qp, form, monkeypatch)
    first = kept["forms"][forms[0]][0]
    for form in forms[1:]:
        out = kept["forms"][form][0]
        bad = np.nonzero(out != first)[0]
        assert bad.size == 0, (case, forms[0], form, [((K.NAMES + K.DERIVED_NAMES * 2)[k], first[k], out[k]) for k in bad])


# ---- d: the derived numbers at their fallbacks ------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ALL)
@pytest.mark.parametrize("state", ["cold", "negative_ray"])
def test_derived_numbers_at_the_fallbacks(state, form, monkeypatch):
    lp = _lp("255x257", "real")
    S = _create(lp, form, True, monkeypatch)
    n, m = S.n, S.m
    cost = S.get("cost", n)
    if state == "cold":  # x = y = 0 with a zero cost: no slack, both norms below 1e-8
        S.set("cost", np.zeros(n))
        x, y = np.zeros(n), np.zeros(m)
    else:  # c'x < 0: the ray objective of the dual infeasibility certificate is negative
        x, y = -cost, np.random.default_rng(13).standard_normal(m)
    for k, a in (("x", x), ("x_sum", x), ("aty", np.zeros(n)), ("y", y), ("y_sum", y), ("ax", np.zeros(m))):
        S.set(k, a)
    out = _check(S, form)
    S.close()
    want = K.derived(out[:30], False, lp.sense, lp.offset)
    d = dict(zip(K.DERIVED_NAMES, out[30:40]))
    assert np.array_equal(out[30:50], want), (state, form, out[30:50], want)
    if state == "cold":
        assert out[8 + 7] == 0.0 and out[2] + out[8 + 4] + out[8 + 5] == 0.0  # ||x||^2, ||(y, s+, s-)||^2
        assert d["pObj"] == lp.offset == d["dObj"] and d["pInfObj"] == 0.0 and d["dInfObj"] == 0.0
        assert d["pFeas"] > 0.0 and d["dInfRes"] == d["pInfRes"] == 0.0
    else:
        assert d["dInfObj"] < 0.0 and out[8 + 7] > 1e-16


# ---- the test stage itself: nothing outlives a reset ------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["one", "seq"])
def test_a_reset_behind_check_device_restores_everything(form, monkeypatch):
    """check_device on a planted state — then, with a planted memory of the last restart, planted weights of the running sums
    and planted x_last / y_last, the check with restarts allowed (it restarts: iteration 0 is not iLastRestartIter = -5) and
    its host-driven twin check_host — reset(), 80 iterations: the iterates, step sizes, counters and restart bookkeeping of a
    solver that never ran a stage."""
    lp = _lp("255x257", "real")
    a, b = _create(lp, form, True, monkeypatch), _create(lp, form, True, monkeypatch)
    rng = np.random.default_rng(14)
    K.plant(a, "real", rng)
    assert a.stage("check_device", 1)[0] == 1.0
    a.set("x_last", rng.standard_normal(a.n)); a.set("y_last", rng.standard_normal(a.m))
    a.set("step_sums", [2.0, 3.0, 0.5, 0.25])
    a.set("restart_memory", [-5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert a.stage("check_device", 1, init=[1])[0] == 1.0
    rs = a.stage("restart_state", 16)
    assert rs[0] in (1.0, 2.0) and rs[1] == 1.0 and rs[2] == 0.0 and rs[9] == rs[10] == 0.0 and not np.any(a.get("x_sum", a.n))
    a.set("restart_memory", [-5, 1.0, 2.0, 3.0, 4.0, 5.0, 6.0])
    assert a.stage("check_host", 1)[0] == 1.0 and a.stage("restart_state", 16)[1] == 2.0
    a.reset()
    assert np.array_equal(a.stage("restart_state", 16), b.stage("restart_state", 16))
    sa, sb = a.iterate(80), b.iterate(80)
    assert (sa.iters, sa.trials, sa.checks, sa.restarts) == (sb.iters, sb.trials, sb.checks, sb.restarts) and sa.iters == 80
    for k in ("x", "y", "ax", "aty", "x_sum", "y_sum", "x_last", "y_last", "steps"):
        length = 8 if k == "steps" else a.m if k in ("y", "ax", "y_sum", "y_last") else a.n
        assert np.array_equal(a.get(k, length), b.get(k, length)), k
    assert np.array_equal(a.stage("restart_state", 16), b.stage("restart_state", 16))
    a.close(); b.close()
