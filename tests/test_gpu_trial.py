"""ONE trial of solver="pdlp" — primal step, A x+, dual step, A'y+, (QP: N x+), the three or four grid-wide sums, the accept /
reject decision and everything it leaves in the device's state record, the deferred updates of the running sums — in every
single-GPU form that runs it, against the elementwise restatement of tests/trial_cases.py (written from cupdlp_step.c and the
record of decideCore; it knows nothing of blocks, trees or the oracle; tests/test_trial_host.py proves its premises on the CPU).

  form                    switches (read at create)                                  asserted through
  plain                   PERSISTENT=0 FUSED=0: k_decide_primal, A x+, A'y+ (, N x+)   small_loop[0] == 0, fused_form[0] == 0, trial_launches == 3
  fused_cc0 / fused_cc1   SLAB=1, CONST_CACHED=0 / 1: the tail of the fused A'y+        fused_form[0] == 1, [2] == cc, trial_launches == 2
  persistentM[_pina]      XCD_LOCAL / HIER_BARRIER / PRIMAL_IN_A: pdlp_small.hip        small_loop[0] > 0, [1] == M, trial_barriers == 2 / 3
  (a QP with off-diagonal Hessian entries in `plain` is plain_qp, in a persistent form persistent_qp: three barriers)
Every solver asserts the form it runs, and barrier_fallbacks == 0 when it is done.

  a. integer data, no scaling, tau and sigma powers of two: x+, y+, A x+, A'y+, N x+ `==` the restatement; dX2, dY2, inter, qint
     `==` the exact sums (any order gives them: trial_cases.exact_sum), movement and limit `==`; at every size and block-count
     case, one rejected and one accepted trial each.
  b. real data, scaling on: x+ and y+ `==` elementwise from the device's own vectors; every sum within the any-order bound
     (k + 1) 2^-53 sum|term| (1 + 1e-6) of the exactly rounded sum of its k terms; the worst error / bound is printed.
  c. the decision in every situation of trial_cases: all 27 numbers of trial_state `==` decide(planted state, sums); behind a
     rejected trial the current iterate's vectors keep their bits; the power table covers the trial (commError == 0).
  d. the running sums over rejected-(rejected-...-)then-accepted and accepted-then-accepted: x_sum, y_sum and the step sums `==` the
     restatement after every trial, each weight added exactly once; x_avg / y_avg of a check_device behind it `==` sum / weight.
  e. the forms agree bit for bit on every case more than one of them runs.
  f. the stage is the loop's trial: iterate(k) from a planted state leaves the state and the vectors of stage("trial") called
     until the same iteration.

Where the pending weight of x sits differs by form and is no observable of the method: the fused tail has already added it to
x_sum when the stage returns (avgWx == 0), the other forms add it in the next primal step.  Compared is what the reference
holds: x_sum with the pending weight applied (trial_cases.flushed — the same product and sum whichever launch does it)."""
import math

import numpy as np
import pytest

import trial_cases as T
from highs_amd import solver

pytestmark = pytest.mark.gpu

SWITCHES = ("PERSISTENT", "PERSISTENT_QP", "FUSED", "SLAB", "CONST_CACHED", "XCD_LOCAL", "HIER_BARRIER", "PRIMAL_IN_A", "CHECK_SMALL", "GRAPH")
FORMS = {
    "plain": dict(PERSISTENT=0, FUSED=0),
    "fused_cc0": dict(SLAB=1, CONST_CACHED=0),
    "fused_cc1": dict(SLAB=1, CONST_CACHED=1),
    "persistent0": dict(XCD_LOCAL=0, HIER_BARRIER=0, PRIMAL_IN_A=0),
    "persistent0_pina": dict(XCD_LOCAL=0, HIER_BARRIER=0, PRIMAL_IN_A=1),
    "persistent1": dict(XCD_LOCAL=1, PRIMAL_IN_A=0),
    "persistent1_pina": dict(XCD_LOCAL=1, PRIMAL_IN_A=1),
    "persistent2": dict(XCD_LOCAL=0, HIER_BARRIER=1, PRIMAL_IN_A=0),
    "persistent2_pina": dict(XCD_LOCAL=0, HIER_BARRIER=1, PRIMAL_IN_A=1),
}
SMALL = tuple(FORMS)
# which forms a case runs in (the rest cannot hold it: trial_cases.py and DESIGN 4b "not reached")
LP_FORMS = {
    "1x1": SMALL, "255x257": SMALL, "256x256": SMALL,
    "65537x300": ("plain", "fused_cc0", "fused_cc1", "persistent0", "persistent2"),
    "blocks256": ("plain", "persistent0", "persistent2"), "blocks257": ("plain", "persistent0", "persistent2"),
    "wide257": ("plain", "persistent2"), "wide768": ("plain",), "wide769": ("plain",), "wide1024": ("plain",), "wide1025": ("plain",),
}
# a QP with a diagonal Hessian runs wherever the LP runs; with off-diagonal entries there is no fused form and no PINA
QP_SPARSE_FORMS = {"255x257": ("plain", "persistent0", "persistent1", "persistent2"), "256x256": ("plain", "persistent1"),
                   "65537x300": ("plain", "persistent2"), "blocks256": ("plain", "persistent2"), "blocks257": ("plain", "persistent2")}
ITERATE = ("x", "y", "ax", "aty")
_runs = {}


def _create(lp, form, values, monkeypatch, qoff=False):
    for k in SWITCHES:
        monkeypatch.delenv("PDLP_MI355X_" + k, raising=False)
    for k, v in FORMS[form].items():
        monkeypatch.setenv("PDLP_MI355X_" + k, str(v))
    S = solver.DeviceSolver(lp, **T.options(values))
    loop, fused, launches = S.stage("small_loop", 3), S.stage("fused_form", 9), int(S.stage("trial_launches", 1)[0])
    what = (lp.model_name, form, loop.tolist(), fused.tolist(), launches)
    if form == "plain":
        assert loop[0] == 0 and fused[0] == 0 and launches == 3, what
    elif form.startswith("fused"):
        assert fused[0] == 1 and fused[2] == FORMS[form]["CONST_CACHED"] and fused[7] > 0 and launches == 2 and loop[0] == 0, what
    else:
        mode, pina = int(form[len("persistent")]), form.endswith("_pina")
        assert loop[0] > 0 and int(loop[1]) == mode and launches == 0 and fused[0] == 0, what
        assert int(S.stage("trial_barriers", 1)[0]) == (2 if pina and not qoff else 3), what
    return S


def _done(S):
    assert S.stage("barrier_fallbacks", 1)[0] == 0.0
    S.close()


def _names(S):
    return list(ITERATE) + (["nx"] if T.K._has(S, "nx") else [])


def _length(S, k):
    return S.m if k.split("_")[0] in ("y", "ax") else S.n


def _read(S):
    names = _names(S)
    out = {k: S.get(k, _length(S, k)) for k in names + [k + "_next" for k in names] + ["x_sum", "y_sum"]}
    return out


def _state(S):
    return T.state_dict(S.get("trial_state", 27))


def _set_state(S, over):
    """Plants `over` on top of the state the solver holds; returns the state as the device now has it.  The push keeps the power
    table ahead of the planted trial counter by refreshPowTable's rule."""
    was = _state(S)
    want = dict(was, **over)
    S.set("trial_state", T.state_array(want))
    now = _state(S)
    base, count = T.pow_table_after_push(want["nTrials"], was["powBase"], was["powCount"])
    assert now == dict(want, powBase=base, powCount=count, pending=0, commError=0), (now, want)
    assert T.covered(now)
    return now


def _plant(S, lp, values, qp, kind, seed=3):
    """Plants an iterate (trial_cases.planted_iterate; integer mode: also a diagonal Hessian that keeps the prox division on the
    grid) and returns everything the trial will read, as the device holds it."""
    n, m = S.n, S.m
    data = {k: S.get(k, m if k == "rhs" else n) for k in ("cost", "rhs", "lower", "upper")}
    data["nx"] = qp == "sparse"
    v = T.planted_iterate(lp, data, values, np.random.default_rng(seed), S.n_eqs, kind)
    if qp and values == "integer":
        S.set("qdiag", T.dyadic_qdiag(n, np.random.default_rng(seed + 1)))
    for k, a in v.items():
        S.set(k, a)
    held = {k: S.get(k, _length(S, k)) for k in v}
    for k, a in v.items():
        assert np.array_equal(held[k].view(np.uint64), np.ascontiguousarray(a).view(np.uint64)), k
    held.update({k: data[k] for k in ("cost", "rhs", "lower", "upper")})
    if qp:
        held["qdiag"] = S.get("qdiag", n)
    assert ("nx" in held) == (qp == "sparse")
    return held


def _bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def _trial(S, form, held, planted, stage="trial_as_is"):
    """One trial from the planted state on the held iterate.  Returns the device's trial point (None where the form has already
    overwritten it), its state, everything read back, and the running sums as the reference holds them."""
    before = _read(S)
    for k in _names(S) + ["x_sum", "y_sum"]:
        assert _bits(before[k], held[k]), k
    S.stage(stage, 10)
    state = _state(S)
    after = _read(S)
    acc = state["lastAccepted"] == 1
    fused = form.startswith("fused")
    point = {k: after[k if acc else k + "_next"] for k in _names(S)}
    if fused and not acc:
        point["x"] = None  # the tail has taken the next trial's primal step into the same buffer
    if not acc:  # a rejected trial leaves the current iterate alone
        for k in _names(S):
            assert _bits(after[k], before[k]), (form, k)
    elif not fused:  # an accepted one leaves the old iterate in the other buffers
        for k in _names(S):
            assert _bits(after[k + "_next"], before[k]), (form, k)
    # the running sums: the trial's primal and dual step applied the weights that were pending when it started
    x_sum = T.flushed(held["x_sum"], held["x"], planted["avgWx"])
    y_sum = T.flushed(held["y_sum"], held["y"], planted["avgW"])
    assert _bits(after["y_sum"], y_sum), form
    if fused:
        assert state["avgWx"] == 0.0 or state["halted"], (form, state)
    else:
        assert _bits(after["x_sum"], x_sum), form
    return point, state, after, (x_sum, y_sum)


def _assert_state(state, want, form, what, after=None, sums_ref=None):
    """All numbers of trial_state against the restated decision.  avgWx: the fused tail has consumed it (see the module
    docstring); then x_sum must already carry it."""
    fused = form.startswith("fused")
    for k in T.STATE:
        if k == "avgWx" and fused and not state["halted"]:
            continue
        assert state[k] == want[k], (what, form, k, state[k], want[k], state, want)
    assert state["commError"] == 0 and T.covered(state)
    if after is not None:
        x_sum, _ = sums_ref
        x_cur = after["x"]
        assert _bits(T.flushed(after["x_sum"], x_cur, state["avgWx"]), T.flushed(x_sum, x_cur, want["avgWx"])), (what, form, "x_sum")


def _sums_of(state):
    return {k: state[k] for k in ("dX2", "dY2", "inter", "qint")}


# ---- a: integer data at every size and block count ---------------------------------------------------------------------------------
def _run_exact(case, qp, form, monkeypatch):
    key = ("exact", case, qp)
    kept = _runs.setdefault(key, {})
    if form in kept:
        return kept
    lp = T.lp_of(case, "integer", qp)
    S = _create(lp, form, "integer", monkeypatch, qoff=qp == "sparse")
    tau, sigma = 2.0**-4, 2.0**-5
    out = []
    _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=1.0))
    held = _plant(S, lp, "integer", qp, "natural")
    nxt, sums = T.restate_trial(lp, held, tau, sigma, S.n_eqs)
    lim = T.limit_of(sums, T.BASE["beta"])
    for eta in (lim * 2.0, lim):  # rejected, then — from the same iterate — accepted
        planted = _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=eta))
        for k in ("x", "y", "ax", "aty", "nx", "x_sum", "y_sum"):  # (the fused tail writes x_next: nothing else has changed)
            if k in held:
                S.set(k, held[k])
        point, state, after, ref_sums = _trial(S, form, held, planted)
        want = T.decide(planted, sums["dX2"], sums["dY2"], sums["inter"], sums["qint"])
        assert want["lastAccepted"] == (eta == lim)
        for k, a in point.items():
            if a is not None:
                bad = np.nonzero(a != nxt[k])[0]
                assert len(bad) == 0, (case, qp, form, k + "+", bad[:8], a[bad[:8]], nxt[k][bad[:8]])
        assert _sums_of(state) == sums, (case, qp, form, _sums_of(state), sums)
        _assert_state(state, want, form, (case, qp, eta), after, ref_sums)
        out.append((state, after))
    _done(S)
    kept[form] = out
    return kept


LP_PARAMS = [(c, None, f) for c, forms in LP_FORMS.items() for f in forms]
DIAG_PARAMS = [(c, "diag", f) for c in ("1x1", "255x257", "65537x300") for f in LP_FORMS[c]]
SPARSE_PARAMS = [(c, "sparse", f) for c, forms in QP_SPARSE_FORMS.items() for f in forms]


@pytest.mark.parametrize("case,qp,form", LP_PARAMS + DIAG_PARAMS + SPARSE_PARAMS)
def test_integer_data_trial_is_exact(case, qp, form, monkeypatch):
    _run_exact(case, qp, form, monkeypatch)


# ---- b: real data ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,qp,form", LP_PARAMS + DIAG_PARAMS + SPARSE_PARAMS)
def test_real_data_sums_within_the_any_order_bound(case, qp, form, monkeypatch):
    lp = T.lp_of(case, "real", qp)
    S = _create(lp, form, "real", monkeypatch, qoff=qp == "sparse")
    tau, sigma = 0.05, 0.03
    _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=1.0))
    held = _plant(S, lp, "real", qp, "natural")
    worst = {}
    for eta in (1e300, 1e-300):  # rejected whatever the sums are (they are finite), then accepted
        planted = _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=eta))
        for k in ("x", "y", "ax", "aty", "nx", "x_sum", "y_sum"):
            if k in held:
                S.set(k, held[k])
        point, state, after, ref_sums = _trial(S, form, held, planted)
        x_next = T.primal_step(held["x"], held["aty"], held["cost"], held["lower"], held["upper"], tau, held.get("qdiag"), held.get("nx"))
        if point["x"] is not None:
            assert np.array_equal(point["x"], x_next), (case, qp, form, "x+")
        point["x"] = x_next
        assert np.array_equal(point["y"], T.dual_step(held["y"], held["ax"], point["ax"], held["rhs"], sigma, S.n_eqs)), (case, qp, form, "y+")
        terms = T.sum_terms(held, point)
        for k, t in terms.items():
            ref, bound = T.any_order_bound(t)
            err = abs(state[k] - ref)
            worst[k] = max(worst.get(k, 0.0), err / bound if bound > 0 else 0.0)
            assert err <= bound, (case, qp, form, k, state[k], ref, err, bound)
        if "qint" not in terms:
            assert state["qint"] == 0.0
        want = T.decide(planted, state["dX2"], state["dY2"], state["inter"], state["qint"])
        assert want["lastAccepted"] == (eta < 1.0)
        _assert_state(state, want, form, (case, qp, eta), after, ref_sums)
    print("trial sums, worst error / any-order bound:", case, qp, form, {k: "%.3g" % v for k, v in worst.items()})
    _done(S)


# ---- c: the decision in every situation ------------------------------------------------------------------------------------------
def _run_situation(name, qp, form, monkeypatch, solvers):
    key = ("situation", name, qp)
    kept = _runs.setdefault(key, {})
    if form in kept:
        return kept
    lp = T.lp_of("255x257", "integer", qp)
    if (qp, form) not in solvers:
        solvers[qp, form] = _create(lp, form, "integer", monkeypatch, qoff=qp == "sparse")
    S = solvers[qp, form]
    kind, tau, sigma = T.ALL_SITUATIONS[name][:3]
    _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=1.0))
    held = _plant(S, lp, "integer", qp, kind)
    nxt, sums = T.restate_trial(lp, held, tau, sigma, S.n_eqs)
    planted = _set_state(S, {k: v for k, v in T.situation_state(name, sums).items() if k not in ("powBase", "powCount")})
    if name == "trials_12288":  # (the situations run in order on one solver: 12287 was served by the table based at 0 or 1)
        assert planted["powBase"] == 12288
    point, state, after, ref_sums = _trial(S, form, held, planted)
    assert _sums_of(state) == sums, (name, qp, form, _sums_of(state), sums)
    claims, want = T.claims(name, planted, _sums_of(state))
    assert all(claims.values()), (name, qp, form, claims)
    _assert_state(state, want, form, (name, qp), after, ref_sums)
    kept[form] = (state, after)
    return kept


def _situation_forms(qp):
    return QP_SPARSE_FORMS["255x257"] if qp == "sparse" else SMALL


def _situation_names(qp):
    return [s for s in T.ALL_SITUATIONS if not ((s in T.QP_SITUATIONS and qp != "sparse") or (s in T.LP_ONLY and qp == "sparse"))]


@pytest.fixture(scope="module")
def solvers():
    held = {}
    yield held
    for S in held.values():
        S.close()


@pytest.mark.parametrize("name,qp,form", [(s, qp, f) for qp in (None, "diag", "sparse") for f in _situation_forms(qp) for s in _situation_names(qp)])
def test_decision_in_every_situation(name, qp, form, monkeypatch, solvers):
    _run_situation(name, qp, form, monkeypatch, solvers)
    assert solvers[qp, form].stage("barrier_fallbacks", 1)[0] == 0.0


def test_power_table_follows_the_planted_trial_counter(monkeypatch):
    """The refresh edge on one solver, in order: 12287 is the last counter the first table serves, 12288 the first that renews it."""
    S = _create(T.lp_of("255x257", "integer"), "plain", "integer", monkeypatch)
    assert (_state(S)["powBase"], _state(S)["powCount"]) == (0, T.POW_WINDOW)
    for n_trials, want in ((1, 0), (12287, 0), (12288, 12288), (12287, 12287), (10**6, 10**6), (0, 0)):
        now = _set_state(S, dict(nTrials=n_trials))
        assert (now["powBase"], now["powCount"]) == (want, T.POW_WINDOW), (n_trials, now)
    _done(S)


# ---- d: the running sums over two trials -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "fused_cc1", "persistent0", "persistent1_pina", "persistent2"])
@pytest.mark.parametrize("qp", [None, "sparse"])
@pytest.mark.parametrize("first", ["rejected", "accepted"])
def test_running_sums_over_two_trials(first, qp, form, monkeypatch):
    if qp == "sparse" and form not in QP_SPARSE_FORMS["255x257"]:
        form = {"fused_cc1": "plain", "persistent1_pina": "persistent1"}[form]
    lp = T.lp_of("255x257", "integer", qp)
    S = _create(lp, form, "integer", monkeypatch, qoff=qp == "sparse")
    tau, sigma = 2.0**-4, 2.0**-5
    _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=1.0))
    held = _plant(S, lp, "integer", qp, "natural")
    sums = T.restate_trial(lp, held, tau, sigma, S.n_eqs)[1]
    lim = T.limit_of(sums, T.BASE["beta"])
    planted = _set_state(S, dict(T.BASE, tau=tau, sigma=sigma, eta=lim * 2.0 if first == "rejected" else lim / 1024.0, avgW=0.375, avgWx=0.375))
    pattern = []
    # x_ref, y_ref: the sums as the reference holds them; wx, w: the weights still to be applied to the current iterate
    x_ref, y_ref, wx, w = held["x_sum"], held["y_sum"], planted["avgWx"], planted["avgW"]
    state = planted
    for trial in range(8 if first == "rejected" else 2):  # (a rejected trial's smaller step may be rejected again: on to the first accepted one)
        before = _read(S)
        # the weights pending when the trial starts land now, once, on the iterate it starts from
        x_ref, y_ref = T.flushed(x_ref, before["x"], wx), T.flushed(y_ref, before["y"], w)
        S.stage("trial_as_is", 10)
        now, after = _state(S), _read(S)
        want = T.decide(state, now["dX2"], now["dY2"], now["inter"], now["qint"])
        wx, w = want["avgWx"], want["avgW"]
        pattern.append(now["lastAccepted"])
        _assert_state(now, want, form, (first, qp, trial), after, (x_ref, y_ref))
        assert _bits(after["y_sum"], y_ref), (first, qp, form, trial)
        if not form.startswith("fused"):
            assert _bits(after["x_sum"], x_ref), (first, qp, form, trial)
        state = now
        if first == "rejected" and now["lastAccepted"]:
            break
    assert pattern == ([0] * (len(pattern) - 1) + [1] if first == "rejected" else [1, 1]) and len(pattern) >= 2, (first, qp, form, pattern)
    # the check behind it flushes what is pending and divides by the step sums
    assert state["nIter"] < 10
    assert S.stage("check_device", 1)[0] == 1.0
    end = _state(S)
    assert end["avgW"] == end["avgWx"] == 0.0 and end["sumPrimalStep"] == state["sumPrimalStep"] and end["sumDualStep"] == state["sumDualStep"]
    x_sum, y_sum = S.get("x_sum", S.n), S.get("y_sum", S.m)
    assert _bits(x_sum, T.flushed(x_ref, after["x"], wx)) and _bits(y_sum, T.flushed(y_ref, after["y"], w))
    assert _bits(S.get("x_avg", S.n), T.average(x_sum, end["sumPrimalStep"])) and _bits(S.get("y_avg", S.m), T.average(y_sum, end["sumDualStep"]))
    _done(S)


# ---- e: the forms agree bit for bit ----------------------------------------------------------------------------------------------
def _assert_same(kept, what):
    forms = list(kept)
    (s0, a0) = kept[forms[0]]
    for f in forms[1:]:
        s1, a1 = kept[f]
        for k in T.STATE:
            if k in ("avgWx", "powBase", "powCount"):  # (where the pending weight sits; the table's base follows each solver's own pushes)
                continue
            assert s0[k] == s1[k] or (isinstance(s0[k], float) and math.isnan(s0[k]) and math.isnan(s1[k])), (what, forms[0], f, k, s0[k], s1[k])
        names = [k for k in a0 if not k.endswith("_next") and k != "x_sum"] + [k for k in a0 if k.endswith("_next") and k != "x_next"]
        for k in names:
            assert _bits(a0[k], a1[k]), (what, forms[0], f, k)
        assert _bits(T.flushed(a0["x_sum"], a0["x"], s0["avgWx"]), T.flushed(a1["x_sum"], a1["x"], s1["avgWx"])), (what, forms[0], f, "x_sum")
        if not (forms[0].startswith("fused") or f.startswith("fused")):
            assert _bits(a0["x_next"], a1["x_next"]) and s0["avgWx"] == s1["avgWx"], (what, forms[0], f)


@pytest.mark.parametrize("case,qp", [(c, None) for c, f in LP_FORMS.items() if len(f) > 1] + [("255x257", "diag")] + [(c, "sparse") for c in QP_SPARSE_FORMS])
def test_forms_agree_on_the_exact_cases(case, qp, monkeypatch):
    forms = QP_SPARSE_FORMS[case] if qp == "sparse" else LP_FORMS[case]
    for form in forms:
        kept = _run_exact(case, qp, form, monkeypatch)
    for trial in (0, 1):
        _assert_same({f: kept[f][trial] for f in forms}, (case, qp, trial))


@pytest.mark.parametrize("qp", [None, "diag", "sparse"])
def test_forms_agree_in_every_situation(qp, monkeypatch, solvers):
    for name in _situation_names(qp):
        for form in _situation_forms(qp):
            kept = _run_situation(name, qp, form, monkeypatch, solvers)
        _assert_same({f: kept[f] for f in _situation_forms(qp)}, (name, qp))


# ---- f: the stage is the loop's trial ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("qp,form", [(None, f) for f in SMALL] + [("sparse", f) for f in QP_SPARSE_FORMS["255x257"]])
def test_stage_is_the_loops_trial(qp, form, monkeypatch):
    """From iteration 41 (no check iteration before 80) with the solver's own initial step sizes on a random iterate: three
    iterations by the fixed-work loop — one persistent launch, or launches with spare trials, up to the halt at 44 — and by
    stage("trial") until the counter says 44; rejected trials are part of both."""
    lp = T.lp_of("255x257", "real", qp)
    got = []
    for how in ("loop", "stage"):
        S = _create(lp, form, "real", monkeypatch, qoff=qp == "sparse")
        _set_state(S, dict(nIter=41, nTrials=41, cur=1))
        _plant(S, lp, "real", qp, "natural")
        if how == "loop":
            st = S.iterate(3)
            assert (st.iters, st.checks, st.restarts) == (3, 0, 0)
            trials = st.trials
        else:
            trials = 0
            while _state(S)["nIter"] < 44:
                S.stage("trial", 10)
                trials += 1
                assert trials <= 40
        state, after = _state(S), _read(S)
        assert state["nIter"] == 44
        got.append((trials, state, after))
        _done(S)
    (ta, sa, va), (tb, sb, vb) = got
    print(form, qp, "trials", ta, tb)
    assert ta == tb
    for k in T.STATE:
        if k not in ("avgWx", "halted", "haltIter", "pending", "powBase", "powCount"):
            assert sa[k] == sb[k], (form, qp, k, sa[k], sb[k])
    for k in _names_of(va):
        assert _bits(va[k], vb[k]), (form, qp, k)
    assert _bits(va["y_sum"], vb["y_sum"])
    assert _bits(T.flushed(va["x_sum"], va["x"], sa["avgWx"]), T.flushed(vb["x_sum"], vb["x"], sb["avgWx"]))


def _names_of(v):
    return [k for k in ITERATE + ("nx",) if k in v]


# ---- the hooks themselves ----------------------------------------------------------------------------------------------------------
def test_trial_state_hooks(monkeypatch):
    S = _create(T.lp_of("255x257", "real"), "plain", "real", monkeypatch)
    with pytest.raises(RuntimeError):
        S.get("trial_state", 26)
    state = _state(S)
    assert (state["nIter"], state["nTrials"], state["cur"], state["halted"], state["haltIter"], state["adaptive"]) == (0, 0, 0, 0, T.INT_MAX, 1)
    assert state["eta"] == math.sqrt(state["primalStep"] * state["dualStep"]) and state["tau"] == state["eta"] / math.sqrt(state["beta"])
    steps = S.get("steps", 8)
    assert (steps[0], steps[1], steps[2], steps[3]) == (state["tau"], state["sigma"], state["beta"], state["eta"])
    # stage "trial" overwrites a planted halt, trial_as_is keeps it; a halted device takes no trial
    _set_state(S, dict(haltIter=0, halted=1))
    before = _state(S)
    S.stage("trial_as_is", 10)
    assert _state(S) == before
    S.stage("trial", 10)
    now = _state(S)
    assert now["nTrials"] == 1 and now["haltIter"] == T.INT_MAX and now["halted"] == 0
    _done(S)
    # solver="hipdlp" has another state record (halpern_state): the names mean nothing there
    H = solver.DeviceSolver(lp=T.lp_of("255x257", "real"), solver="hipdlp")
    with pytest.raises(RuntimeError):
        H.get("trial_state", 27)
    with pytest.raises(RuntimeError):
        H.set("trial_state", T.state_array(state))
    with pytest.raises(RuntimeError):
        H.stage("trial_as_is", 10)
    H.close()
