"""What a check iteration does once its numbers are known — the restart — in all three forms that carry it out, against the
restatement of tests/restart_cases.py (from the text of cuPDLP-C, not from the product's code):

  form "one"   phases D, V, W of the one-launch check (pdlp_check.hip checkSmallBody)       stage check_device, init = [1]
  form "seq"   k_check_decide, k_restart_vec, k_restart_finish behind the statistics        stage check_device, init = [1]
  form "host"  Solver::restartIterate behind computeAverage / computeResiduals              stage check_host
Forms are created and asserted as in tests/test_gpu_check_stats.py (check_launches, small_loop).  Every test plants a state
(restart_cases.plant_restart: vectors, x_last / y_last, the weights of the running sums, the memory of the last restart and
candidate) that reaches exactly one branch of the decision — tests/test_restart_host.py proves that on the CPU — reads it back,
runs ONE check with restarts allowed and reads everything again.

  a. integer data, no scaling: the kind, every vector (bit patterns), restart_state and steps `==` decide / expected_vectors /
     finish, the latter fed with the exact integers ||x - x_last||^2, ||y - y_last||^2.
  b. real data, scaling on: vectors and memory as in a; the decision's inputs are the check's own 20 derived numbers (pinned by
     tests/test_gpu_check_stats.py); beta within beta_ref (1 +- tol), beta_ref from the exactly rounded sums (TOLERANCE
     below); tau, sigma, eta, primalStep, dualStep `==` the float64 chain evaluated from the device's beta.
  c. the three forms on the same planted state: every vector, every number of steps and restart_state bit-identical.
  d. behind a running solve the stage is the loop's own restart: a solver stopped at 40, restarted by the stage and run on to
     80 has the bits of one that ran straight through.  (Its second stretch enters with a check at 40 again, which finds
     it == iLastRestartIter, records the restarted iterate's numbers — the bits the restart recorded: same vectors, same tree —
     and restarts nothing: one check more, nothing else differs.)
  e. no restart really is none.

The stage's control record is the fixed-work loop's with target nIter + 1, in both stages: the next halt of the schedule is
clipped to it, haltIter == nIter + 1.

TOLERANCE of b (u = 2^-53).  Both sides evaluate lg = 0.5 log(dD / dP) + 0.5 log(sqrt(beta)), beta' = exp(lg) exp(lg) with the
same functions (exp / log within one ulp of the true value: tests/test_host.py) from the same beta; they differ in dP2, dD2: the
device's sums lie within (len + 1) u (1 + 1e-6) of the exactly rounded ones, relative (non-negative terms).
  dD / dP        half the relative difference of each sum: 1/2 ((n + 1) + (m + 1)) u (1 + 1e-6) in all; per side two square
                 roots and a division: 3 u
  0.5 log(.)     the absolute error of the logarithm is the relative one of its argument, halved: 1.5 u; its own error, below one
                 ulp <= 2 u |log|, with |0.5 log| <= 8 (asserted): 16 u
  the sum        u |lg| <= 8 u (|lg| <= 8, asserted); 0.5 log(sqrt(beta)) is the same number on both sides
  exp(lg)^2      relative 2 (25.5 u) + two evaluations within one ulp (2 u each) + the product (u): 56 u per side
so c = 112 and tol = 1/2 ((n + 1) + (m + 1)) u (1 + 1e-6) + 112 u."""
import math

import numpy as np
import pytest

import check_cases as K
import lpgen
import restart_cases as R
from highs_amd import solver
from test_gpu_check_stats import ALL, CASES, _create, _lp, _options

pytestmark = pytest.mark.gpu

U = 2.0**-53
C_SCALAR = 112
THREE = ("artificial_avg", "artificial_cur", "sufficient")
DECAY = ("sufficient", "not_sufficient_not_necessary", "necessary", "too_slow", "artificial_edge_25", "artificial_edge_26")
SIZED = ("1x1", "256x256", "65537x300", "65537x300thin", "196608x196609", "524288x524289")
LP_KEYS = [("255x257", s) for s in R.SITUATIONS] + [(c, s) for c in SIZED for s in THREE] + [("grid64", "artificial_avg"), ("wide16385", "artificial_avg")]
LP_PARAMS = [(c, s, f) for c, s in LP_KEYS for f in CASES[c][1]]
QP_KEYS = [(c, qp, s) for c in ("255x257", "65537x300") for qp in ("diag", "sparse") for s in ("artificial_avg", "artificial_cur", "first")]
QP_PARAMS = [(c, qp, s, f) for c, qp, s in QP_KEYS for f in CASES[c][1]]
_prepared, _runs = {}, {}


def _form_of(case, values):
    key = (case, values)
    if key not in _prepared:
        _prepared[key] = solver.Prepared(_lp(case, values), **_options(values))
    return _prepared[key]


def _names(S):
    names = ["x", "y", "ax", "aty", "x_sum", "y_sum", "x_last", "y_last"] + (["nx"] if K._has(S, "nx") else [])
    return names, ["x_avg", "y_avg", "ax_avg", "aty_avg"] + (["nx_avg"] if K._has(S, "nx") else [])


def _length(S, k):
    return S.m if k.split("_")[0] in ("y", "ax") else S.n


def _read(S, names):
    return {k: S.get(k, _length(S, k)) for k in names}


def _scalars(S):
    steps, rs = S.get("steps", 8), S.stage("restart_state", 16)
    state = dict(zip(R.STEPS, steps))
    state.update(sumDualStep=rs[10], iLast=int(rs[2]), nRestarts=int(rs[1]), nChecks=int(rs[14]))
    return steps, rs, state


def _check(S, form):
    if form == "host":
        assert S.stage("check_host", 1)[0] == 1.0
    else:
        assert S.stage("check_device", 1, init=[1])[0] == 1.0  # the record's `ran`


def _run(case, values, qp, situation, form, monkeypatch):
    """The situation on the case in one form: run once, kept.  Every form must have held the same planted state."""
    key = (case, values, qp, situation)
    kept = _runs.setdefault(key, {"forms": {}})
    if form in kept["forms"]:
        return kept
    s = R.SITUATIONS[situation]
    lp = _lp(case, values, qp)
    off = _options(values).get("pdlp_features_off", 0) | s.options.get("pdlp_features_off", 0)
    S = _create(lp, form, "one" in CASES[case][1], monkeypatch, **(dict(pdlp_features_off=off) if off else {}))
    P = _form_of(case, values) if situation in DECAY else None
    vec, memory, der, beta = R.plant_restart(S, situation, values, np.random.default_rng(31), P=P, data=CASES[case][2])
    names, avgs = _names(S)
    before = _read(S, names)
    for k, a in vec.items():
        assert R.same_bits(before[k], a), (case, situation, form, k)
    steps0, rs0, state0 = _scalars(S)
    assert tuple(rs0[2:9]) == tuple(memory) and rs0[9] == rs0[10] == 1.0 and rs0[11] == rs0[12] == 0.0 and steps0[2] == beta
    it = s.it
    _check(S, form)
    after = _read(S, names + avgs)
    stats = S.stage("check_stats", 50)
    steps1, rs1, _ = _scalars(S)
    S.close()
    out = dict(after=after, stats=stats, steps=steps1, rs=rs1)
    if "before" not in kept:
        kept.update(before=before, state0=state0, memory=memory, der=der, beta=beta, it=it, n=len(before["x"]), m=len(before["y"]),
                    sense=lp.sense, offset=lp.offset, qp=qp is not None, adaptive=not s.options)
    else:
        assert kept["state0"] == state0 and all(R.same_bits(before[k], kept["before"][k]) for k in before), (case, situation, form)
    kept["forms"][form] = out
    return kept


def _assert_restart(kept, form, values, situation, what):
    s = R.SITUATIONS[situation]
    out, before, state0, it = kept["forms"][form], kept["before"], kept["state0"], kept["it"]
    after, stats, steps, rs = out["after"], out["stats"], out["steps"], out["rs"]
    integer = values == "integer"
    # the decision, from the check's own derived numbers (themselves `==` check_cases.derived of its 30 sums)
    der = stats[30:50]
    assert np.array_equal(der, K.derived(stats[:30], kept["qp"], kept["sense"], kept["offset"])), what
    if integer and kept["der"] is not None:  # the CPU's numbers, from the planted vectors: exact integers in, the same bits out
        assert np.array_equal(der, kept["der"]), (what, der, kept["der"])
    taken = []
    kind, memory = R.decide(der[:10], der[10:], kept["beta"], it, kept["memory"], taken)
    print(what, form, "branch", taken[0][0], "kind", kind, taken[0][1])
    assert (taken[0][0], kind) == (s.branch, s.kind), (what, taken)  # the device's numbers reach the situation's branch too
    if "muCur" in taken[0][1]:
        mu = taken[0][1]
        assert max(mu["muCur"], mu["muAvg"]) >= 10.0 * min(mu["muCur"], mu["muAvg"]), (what, mu)
    assert int(rs[0]) == kind, (what, form, rs[0], kind)
    # the vectors
    v = dict(before, **{k: after[k] for k in after if k.endswith("_avg")})
    assert R.same_bits(v["x_avg"], before["x_sum"]) and R.same_bits(v["y_avg"], before["y_sum"])  # (weights one, nothing pending)
    want = R.expected_vectors(v, before["x_last"], before["y_last"], kind, integer=integer)
    for k in before:
        assert R.same_bits(after[k], want[k]), (what, form, k, np.nonzero(after[k] != want[k])[0][:8])
    if "nx" in before and kind:
        assert R.same_bits(after["nx"], after["nx_avg"] if kind == 2 else before["nx"])
    # the scalars
    got = dict(zip(R.STEPS, steps))
    if integer or not kind:
        fin = R.finish(state0, kind, want["dP2"].exact if kind else 0, want["dD2"].exact if kind else 0, kept["adaptive"], it)
        if kind:
            assert 0 <= want["dP2"].exact < 2**53 and 0 <= want["dD2"].exact < 2**53
    else:
        dP2, dD2 = want["dP2"].fsum, want["dD2"].fsum
        ref = R.finish(state0, kind, dP2, dD2, kept["adaptive"], it)
        tol = 0.5 * ((kept["n"] + 1) + (kept["m"] + 1)) * U * (1 + 1e-6) + C_SCALAR * U
        lg = R.log_beta_update(state0["beta"], dP2, dD2)
        if lg is not None:
            half = (0.5 * R.det_exp_log(math.sqrt(dD2) / math.sqrt(dP2))[1], 0.5 * R.det_exp_log(math.sqrt(state0["beta"]))[1])
            assert abs(lg) <= 8.0 and abs(half[0]) <= 8.0 and abs(half[1]) <= 8.0, (what, lg, half)
        print(what, form, "beta", got["beta"], "beta_ref", ref["beta"], "relative difference", abs(got["beta"] - ref["beta"]) / ref["beta"], "tol", tol)
        assert abs(got["beta"] - ref["beta"]) <= tol * ref["beta"], (what, form, got["beta"], ref["beta"], tol)
        assert (got["beta"] == state0["beta"]) == (lg is None)
        fin = R.step_chain(state0, got["beta"], kept["adaptive"])  # the float64 chain from the device's beta
        fin.update(sumPrimalStep=0.0, sumDualStep=0.0, iLast=it, nRestarts=state0["nRestarts"] + 1)
    print(what, form, "state before", {k: repr(float(t)) for k, t in state0.items()}, "after", {k: repr(float(t)) for k, t in got.items()},
          "distances", kind and (want["dP2"].fsum, want["dD2"].fsum))
    for k in ("beta", "primalStep", "dualStep", "eta", "tau", "sigma", "sumPrimalStep"):
        assert got[k] == fin[k], (what, form, k, got[k], fin[k])
    assert got["avgW"] == 0.0
    if situation == "still":
        assert got["beta"] == state0["beta"] and kind == 1
    want_rs = [kind, fin["nRestarts"], fin["iLast"], *memory[1:7], fin["sumPrimalStep"], fin["sumDualStep"], 0.0, 0.0, it + 1, state0["nChecks"] + 1, it]
    assert list(rs) == [float(t) for t in want_rs], (what, form, dict(zip(R.RESTART_STATE, zip(rs, want_rs))))


# ---- a, b: every form, every situation at 255 x 257, three situations at every size ---------------------------------------------
@pytest.mark.parametrize("case,situation,form", LP_PARAMS)
def test_integer_data_restart_is_exact(case, situation, form, monkeypatch):
    _assert_restart(_run(case, "integer", None, situation, form, monkeypatch), form, "integer", situation, case + " " + situation)


@pytest.mark.parametrize("case,situation,form", LP_PARAMS)
def test_real_data_restart(case, situation, form, monkeypatch):
    _assert_restart(_run(case, "real", None, situation, form, monkeypatch), form, "real", situation, case + " " + situation)


@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("case,qp,situation,form", QP_PARAMS)
def test_qp_restart_moves_nx_with_the_iterate(case, qp, situation, form, values, monkeypatch):
    kept = _run(case, values, qp, situation, form, monkeypatch)
    assert ("nx" in kept["before"]) == (qp == "sparse")
    _assert_restart(kept, form, values, situation, case + qp + " " + situation)


# ---- c: the three forms agree bit for bit -----------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("case,qp,situation", [(c, None, s) for c, s in LP_KEYS if len(CASES[c][1]) > 1] + QP_KEYS)
def test_forms_agree_bit_for_bit(case, qp, situation, values, monkeypatch):
    forms = CASES[case][1]
    for form in forms:
        kept = _run(case, values, qp, situation, form, monkeypatch)
    first = kept["forms"][forms[0]]
    for form in forms[1:]:
        out = kept["forms"][form]
        for k in first["after"]:
            assert R.same_bits(first["after"][k], out["after"][k]), (case, situation, forms[0], form, k)
        assert R.same_bits(first["steps"], out["steps"]), (case, situation, form, first["steps"], out["steps"])
        assert R.same_bits(first["rs"], out["rs"]), (case, situation, form, dict(zip(R.RESTART_STATE, zip(first["rs"], out["rs"]))))
        assert R.same_bits(first["stats"], out["stats"])


# ---- e: no restart really is none -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("form", ALL)
@pytest.mark.parametrize("situation", ["first", "not_sufficient_not_necessary", "too_slow"])
def test_no_restart_is_none(situation, form, values, monkeypatch):
    kept = _run("255x257", values, None, situation, form, monkeypatch)
    out, before, state0 = kept["forms"][form], kept["before"], kept["state0"]
    assert int(out["rs"][0]) == 0 and int(out["rs"][1]) == state0["nRestarts"] and int(out["rs"][2]) == state0["iLast"]
    for k in before:  # everything but the averages the flush writes
        assert R.same_bits(out["after"][k], before[k]), (situation, form, k)
    got = dict(zip(R.STEPS, out["steps"]))
    for k in ("sumPrimalStep", "beta", "tau", "sigma", "eta", "primalStep", "dualStep"):
        assert got[k] == state0[k], (situation, form, k)
    assert out["rs"][10] == state0["sumDualStep"] == 1.0 and out["rs"][9] == 1.0
    assert int(out["rs"][13]) == kept["it"] + 1  # the schedule's next halt, clipped to the stage's target nIter + 1
    lr, lc = tuple(out["rs"][3:6]), tuple(out["rs"][6:9])
    cur = tuple(out["stats"][30 + k] for k in (R.PFEAS, R.DFEAS, R.GAP))
    if situation == "first":
        assert lr == cur and lc == cur
    else:
        assert lr == tuple(kept["memory"][1:4]) and lc != tuple(kept["memory"][4:7])  # LC moves, LR stays


# ---- d: behind a running solve ----------------------------------------------------------------------------------------------
def _behind(lp, form, loop_takes_it, monkeypatch, fused=False):
    if fused:
        monkeypatch.delenv("PDLP_MI355X_CHECK_SMALL", raising=False)
        a, b = solver.DeviceSolver(lp), solver.DeviceSolver(lp)
        assert int(a.stage("trial_launches", 1)[0]) == 2 and int(a.stage("check_launches", 1)[0]) == 10
        assert int(a.stage("fused_form", 9)[0]) == 1 and a.stage("fused_form", 9)[7] > 0  # the fused trial on the slab layout
    else:
        a, b = _create(lp, form, loop_takes_it, monkeypatch), _create(lp, form, loop_takes_it, monkeypatch)
    names, avgs = _names(a)
    sa = [a.iterate(40)]
    assert sa[0].iters == 40
    before = _read(a, names)
    steps0, rs0, state0 = _scalars(a)
    assert state0["sumPrimalStep"] > 0.0 and state0["sumDualStep"] > 0.0 and state0["iLast"] < 10
    _check(a, form)
    after = _read(a, names + avgs)
    steps1, rs1, _ = _scalars(a)
    kind = int(rs1[0])
    print(lp.model_name, form, "kind", kind, "iLast before", state0["iLast"], "beta", steps0[2], "->", steps1[2])
    assert kind != 0  # 40 - iLast >= 31 >= 0.36 * 40: the artificial restart, whatever the seed
    if kind == 2:
        for k in ("x", "y", "ax", "aty") + (("nx",) if "nx" in before else ()):
            assert R.same_bits(after[k], after[k + "_avg"]), k
    else:
        for k in ("x", "y", "ax", "aty"):
            assert R.same_bits(after[k], before[k]), k
    assert not np.any(after["x_sum"]) and not np.any(after["y_sum"])
    assert R.same_bits(after["x_last"], after["x"]) and R.same_bits(after["y_last"], after["y"])
    assert rs1[11] == rs1[12] == 0.0 and rs1[9] == rs1[10] == 0.0 and steps1[6] == 0.0
    assert (int(rs1[1]), int(rs1[2]), int(rs1[15]), int(rs1[14])) == (state0["nRestarts"] + 1, 40, 40, state0["nChecks"] + 1)
    sa.append(a.iterate(40))
    sb = b.iterate(80)
    assert sa[1].iters == 40 and sb.iters == 80
    assert sa[0].trials + sa[1].trials == sb.trials and sa[0].restarts + 1 + sa[1].restarts == sb.restarts
    assert sa[0].checks + 1 + sa[1].checks == sb.checks + 1  # (the entry check at 40 of the second stretch: see the module docstring)
    for k in names:
        assert R.same_bits(a.get(k, _length(a, k)), b.get(k, _length(b, k))), (lp.model_name, form, k)
    (st_a, rs_a, _), (st_b, rs_b, _) = _scalars(a), _scalars(b)
    assert R.same_bits(st_a, st_b), (st_a, st_b)
    same = [k for k in range(16) if R.RESTART_STATE[k] not in ("nChecks", "kind")]  # (a's last check is the entry check at 40: kind 0)
    assert R.same_bits(rs_a[same], rs_b[same]) and rs_a[14] == rs_b[14] + 1 and (rs_a[0], rs_b[0]) == (0.0, float(kind)), dict(zip(R.RESTART_STATE, zip(rs_a, rs_b)))
    a.close(); b.close()


@pytest.mark.parametrize("case,form", [("255x257", "one"), ("255x257", "seq"), ("255x257", "host"), ("65537x300", "seq")])
def test_restart_behind_a_running_solve(case, form, monkeypatch):
    _behind(_lp(case, "real"), form, "one" in CASES[case][1], monkeypatch)


def test_restart_behind_a_running_fused_solve(monkeypatch):
    _behind(lpgen.structured_lp(arcs=8192, link_rows=64), "seq", False, monkeypatch, fused=True)
