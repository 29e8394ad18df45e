"""The tail of the fused A'y+ launch (k_spmv_slab<kAtyFused, TWO, CC, ULO>: decision, deferred xSum update, the NEXT trial's
primal step) at the column counts per block where its structure changes — tests/fused_cases.py, whose structural claims are
proven on the host planner in tests/test_fused_cases_host.py.  Every test asserts through stage "fused_form" that the device
runs the instantiation the case was built for; every comparison is `==` / array_equal.

a. One tail step against an elementwise restatement (fused_cases.tail_step: numpy float64 in the kernel's operation order,
   which knows nothing of blocks, registers or the oracle).  x, y and the step sizes are set as test_gpu_parity.
   _trial_step_check sets them, once with steps that are accepted and once with steps that are rejected (3000 / 30: the
   projections bound dx, and eta / limit settles at 1.14 .. 2.0 on these cases); after each of two trials in a row the tail's
   x[cur ^ 1] must equal the restatement, bit for bit (the sign of a zero included), on the x, A'y and tau the decision has
   left.  stage("trial") pushes the state, so BOTH trials start with the stand-alone primal step and nothing here consumes
   what the tail wrote — part b does; what is compared is the tail's own output all the same, since it is the last writer of
   x[cur ^ 1].  The per-block uniform-bound bits and lowerUniform are restated from the device's bounds by bit pattern and
   compared with what the device derived.  Every case runs under CONST_CACHED = 0 and 1.
b. Form against form over 120 iterations (check iterations, restarts and rejected trials inside: the host test asserts them
   on the oracle): the 3-launch form, CONST_CACHED, TOUCH_TAIL, FUSED_COTASKS, GRAPH — the same bits; every case without a
   long column (every bound pattern and the QP included) also against the oracle's solve in the device's reduction order.
c. Bounds written through set("lower" / "upper"): the fused solver follows them like the 3-launch form."""
import numpy as np
import pytest

import fused_cases as F
import oraclelib as O
from highs_amd import solver
from test_gpu_qp_small import _assert_equals_oracle

pytestmark = pytest.mark.gpu

SWITCHES = ("PDLP_MI355X_FUSED", "PDLP_MI355X_CONST_CACHED", "PDLP_MI355X_TOUCH_TAIL", "PDLP_MI355X_FUSED_COTASKS", "PDLP_MI355X_GRAPH")
SWEEP = ["late%d" % T for T in F.LATE_T] + ["two%d" % T for T in F.TWO_T + (F.TWO_MAX,)] + ["inline%d" % (F.TWO_MAX + 1)]
PATTERNS = sorted(set(F.CASES) - set(SWEEP))


def _solver(name, monkeypatch, env=None, **kw):
    """A solver of the case on the slab layout with exactly the switches of `env` set (they are read at create)."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1")
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv("PDLP_MI355X_" + k, str(v))
    lp, opt = F.case(name)
    return solver.DeviceSolver(lp, **opt, **kw)


def _blocks(name):
    lp, _ = F.case(name)
    return F.block_starts(np.diff(lp.a_start))  # (== the planner's blocks: test_fused_cases_host.py)


def _uniform(S, name):
    """(bits per block, lowerUniform, columns with a block-wide lower bound, with a block-wide upper bound), restated from the
    bounds the device holds."""
    return F.block_uniform_bits(S.get("lower", S.n), S.get("upper", S.n), _blocks(name))


def _assert_form(S, name, cc=1, ulo=None, cotasks=True, touch=1):
    """The instantiation the case claims to run: stage "fused_form"."""
    T, variant = F.CASES[name][:2]
    two = variant == "TWO" and cotasks
    form = S.stage("fused_form", 9)
    assert form[8] == F.STATE_BYTES, "sizeof(DevState) is %d, fused_cases.STATE_BYTES (which gives TWO_MAX) says %d" % (form[8], F.STATE_BYTES)
    if ulo is None:
        ulo = _uniform(S, name)[1]
    print(name, "fused_form", form.tolist())
    assert form[0] == 1, "the case does not run the fused trial"
    assert (form[1], form[2], form[3]) == (int(two), cc, int(ulo))
    assert (form[4] > 0) == two and form[5] == int(name in F.HAS_LONG and not two) and form[6] == touch
    assert form[7] == np.diff(_blocks(name)).max() and form[7] >= T  # rowsPerBlock: the most columns a block owns — the last one's, but for T = 128
    return form


# ---- a: one tail step -----------------------------------------------------------------------------------------------------------
def _tail_params():
    return [(name, cc) for name in SWEEP + PATTERNS for cc in (1, 0)]


@pytest.mark.parametrize("name,cc", _tail_params())
def test_the_tail_takes_the_next_primal_step(name, cc, monkeypatch):
    S = _solver(name, monkeypatch, {"CONST_CACHED": cc})
    n, m = S.n, S.m
    bits, all_lower, n_lower, n_upper = _uniform(S, name)
    assert bits[-1] == F.LAST_BITS[F.CASES[name][2]] and all_lower == (F.CASES[name][2] in F.LOWER_UNIFORM)
    _assert_form(S, name, cc, all_lower)
    assert S.stage("uniform_bound_columns", 2).tolist() == [n_lower, n_upper]
    assert S.stage("update_state", 8)[2] == int(all_lower)
    cost, lower, upper = S.get("cost", n), S.get("lower", n), S.get("upper", n)
    qd = S.get("qdiag", n) if F.CASES[name][3] else None
    def check_tail(what):
        now = S.get("steps", 8)[0]
        want = F.tail_step(S.get("x", n), S.get("aty", n), cost, lower, upper, now, qd)
        got = S.get("x_next", n)
        wrong = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]  # (-0.0 is not +0.0)
        assert len(wrong) == 0, (what, wrong[:8], got[wrong[:8]], want[wrong[:8]])

    rng = np.random.default_rng(5)
    free = F.CASES[name][2] == "free"
    for tau, sigma, accepted in ((0.002, 0.001, 1.0), (3000.0, 30.0, 0.0))[:1 if free else 2]:
        x = np.clip(rng.standard_normal(n), lower, upper)
        y = rng.standard_normal(m)
        y[S.n_eqs:] = np.maximum(y[S.n_eqs:], 0.0)
        S.set("x", x); S.set("y", y)
        S.stage("ax"); S.stage("aty")
        S.set("steps", [tau, sigma, sigma / tau])
        for trial in range(2):
            out = S.stage("trial")
            if trial == 0:
                assert out[3] == accepted, (tau, sigma, out[:4])
            check_tail((tau, trial, out[3]))
    if free:
        # Unbounded columns: no step is large enough to be rejected from a random point (dx and dy grow together and the
        # limit tends to eta from above: eta / limit = 0.99 .. 1.00 for tau from 30 to 3e5 at every ratio sigma / tau).  The
        # rejected branch is taken where the solve itself rejects: trials from the iterate after 20 iterations on, each one
        # checked, up to the first rejected one
        S.reset()
        S.iterate(20)
        for trial in range(80):
            out = S.stage("trial")
            check_tail(("after 20 iterations", trial, out[3]))
            if out[3] == 0.0:
                break
        print(name, "first rejected trial after", trial + 1)
        assert out[3] == 0.0
    assert S.stage("barrier_fallbacks", 1)[0] == 0
    S.close()


# ---- b: form against form -------------------------------------------------------------------------------------------------------
VECTORS = (("x", "n"), ("y", "m"), ("x_sum", "n"), ("y_sum", "m"))
_default = {}


def _state(S):
    st = S.iterate(F.ITER_CAP)
    out = {k: S.get(k, getattr(S, d)) for k, d in VECTORS}
    out["steps"] = S.get("steps", 8)
    out["counts"] = np.array([st.iters, st.trials, st.restarts, st.checks])
    return out


def _default_state(name, monkeypatch):
    """120 iterations of the default fused form (computed once per case, shared, never changed)."""
    if name not in _default:
        S = _solver(name, monkeypatch, **F.SOLVE)
        _assert_form(S, name)
        _default[name] = _state(S)
        assert S.stage("barrier_fallbacks", 1)[0] == 0
        S.close()
        c = _default[name]["counts"]
        print(name, "iterations", c[0], "trials", c[1], "restarts", c[2])
        assert c[0] == F.ITER_CAP and c[1] > c[0] and c[2] >= 1
    return _default[name]


def _assert_same_state(a, b, what):
    for k in a:
        assert np.array_equal(a[k], b[k]), (what, k)


@pytest.mark.parametrize("name", SWEEP + PATTERNS)
def test_fused_and_three_launch_forms_give_the_same_bits(name, monkeypatch):
    want = _default_state(name, monkeypatch)
    S = _solver(name, monkeypatch, {"FUSED": 0}, **F.SOLVE)
    assert S.stage("fused_form", 8)[0] == 0 and S.stage("trial_launches", 1)[0] == 3
    _assert_same_state(_state(S), want, name)
    S.close()


FORMS = [(name, {"CONST_CACHED": 0}, dict(cc=0)) for name in ("late8193", "two5121")] + \
        [(name, {"TOUCH_TAIL": 0}, dict(touch=0)) for name in ("two2049", "two5120", "two5121", "two%d" % F.TWO_MAX)] + \
        [(name, {"FUSED_COTASKS": 0}, dict(cotasks=False)) for name in ("two2049", "two5121")] + \
        [(name, {"GRAPH": 0}, {}) for name in ("late8193", "two5121")]


@pytest.mark.parametrize("name,env,form", FORMS, ids=["%s-%s" % (n, "-".join(e)) for n, e, _ in FORMS])
def test_switches_of_the_fused_form_give_the_same_bits(name, env, form, monkeypatch):
    want = _default_state(name, monkeypatch)
    S = _solver(name, monkeypatch, env, **F.SOLVE)
    _assert_form(S, name, **form)
    if "GRAPH" in env:
        assert S.stage("update_state", 8)[3] == 0  # no captured graph
    _assert_same_state(_state(S), want, (name, env))
    assert S.stage("barrier_fallbacks", 1)[0] == 0
    S.close()


@pytest.mark.parametrize("name", [n for n in SWEEP + PATTERNS if n not in F.HAS_LONG])
def test_whole_solve_has_the_oracles_bits(name, monkeypatch):
    lp, opt = F.case(name)
    cpu = O.oracle_solve(lp, device_reduction_order=True, device_layout="slab", **F.SOLVE, **opt)
    assert cpu.num_trials > cpu.num_iter and cpu.num_restarts >= 1
    S = _solver(name, monkeypatch, **F.SOLVE)
    _assert_form(S, name)
    gpu = S.solve()
    assert S.stage("barrier_fallbacks", 1)[0] == 0
    S.close()
    _assert_equals_oracle(gpu, cpu)


# ---- c: bounds written through set ----------------------------------------------------------------------------------------------
def test_bounds_written_through_set_reach_the_fused_tail(monkeypatch):
    name = "late8193_box37"  # unscaled, every column -0.75 .. 1.5: lowerUniform = 1
    lp, _ = F.case(name)
    cut = _blocks(name)
    kw = dict(kkt_tolerance=F.SOLVE["kkt_tolerance"])  # (no iteration limit: 280 iterations in all)
    fused = _solver(name, monkeypatch, **kw)
    plain = _solver(name, monkeypatch, {"FUSED": 0}, **kw)
    untouched = _solver(name, monkeypatch, **kw)
    n, m = fused.n, fused.m
    lower, upper = fused.get("lower", n), fused.get("upper", n)
    assert np.array_equal(lower, lp.col_lower) and np.array_equal(upper, lp.col_upper)
    _assert_form(fused, name, ulo=True)
    assert fused.stage("update_state", 8)[2:4].tolist() == [1, 1]  # lowerUniform, a captured graph
    lower2, upper2 = lower.copy(), upper.copy()
    lower2[cut[-2] + 4096] = -0.5  # the last block's 4097th column: the first one whose x+ the step takes from xbLate[]
    upper2[cut[1]:cut[2]] = np.random.default_rng(7).uniform(0.5, 1.5, cut[2] - cut[1])  # the second block: no shared upper bound

    def write(lo, up):
        for S in (fused, plain):
            S.set("lower", lo); S.set("upper", up)
        bits, all_lower, n_lower, n_upper = _uniform(fused, name)
        _assert_form(fused, name, ulo=all_lower)
        assert fused.stage("update_state", 8)[2:4].tolist() == [int(all_lower), 1]
        assert fused.stage("uniform_bound_columns", 2).tolist() == [n_lower, n_upper]
        return bits, all_lower

    def run(iters, what):
        sf, sp = fused.iterate(iters), plain.iterate(iters)
        assert (sf.iters, sf.trials, sf.restarts) == (sp.iters, sp.trials, sp.restarts), what
        for k, d in VECTORS:
            assert np.array_equal(fused.get(k, getattr(fused, d)), plain.get(k, getattr(plain, d))), (what, k)
        assert np.array_equal(fused.get("steps", 8), plain.get("steps", 8)), what
        x = fused.get("x", n)
        assert np.all(x >= fused.get("lower", n)) and np.all(x <= fused.get("upper", n)), what

    bits, all_lower = write(lower2, upper2)  # after create
    assert not all_lower and bits[1] == 1 and bits[-1] == 2 and np.all(np.delete(bits, [1, len(bits) - 1]) == 3)
    run(40, "changed after create")
    bits, all_lower = write(lower, upper)  # the original bounds back, a graph has run: lowerUniform = 1 again
    assert all_lower and np.all(bits == 3)
    run(40, "restored")
    write(lower2, upper2)  # and changed again behind a graph that has run
    run(80, "changed after 80 iterations")
    write(lower, upper)
    fused.reset()
    a, b = _state(fused), _state(untouched)
    _assert_same_state(a, b, "restored and reset against an untouched solver")
    for S in (fused, plain, untouched):
        assert S.stage("barrier_fallbacks", 1)[0] == 0
        S.close()
