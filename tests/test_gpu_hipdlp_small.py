"""GPU tests of the persistent launch of the HiPDLP path on small LPs (highs_amd/csrc/pdlp_halpern_small.hip): the Halpern steps
2..40 of a block as ONE launch with grid barriers instead of 78 kernel nodes.  The feature changes no bit, so every comparison
here is == / array_equal: against the oracle (oracle/hipdlp_oracle.c) for blocks of steps, against the same library with
PDLP_MI355X_PERSISTENT_HIPDLP=0 for whole solves.  No test makes a launch wait for its timeout."""
import functools
import os

import numpy as np
import pytest

import oraclelib as O
from highs_amd import solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SWITCH = "PDLP_MI355X_PERSISTENT_HIPDLP"
VECS = ("x", "y", "x_next", "y_next")


@functools.lru_cache(maxsize=None)
def _lp(name):
    return L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz"))


@functools.lru_cache(maxsize=None)
def _probe(name, steps, order=None):
    """The oracle's state after `steps` Halpern steps of the first block; computed once, shared, never written to."""
    kw = dict(device_reduction_order=True, device_layout=order) if order else {}
    ref = O.hipdlp_probe(_lp(name), steps, **kw)
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def _stage(S, name):
    return S.stage(name)[0]


def _counters(S):
    return {k: int(_stage(S, k)) for k in ("persistent_launches", "step_barriers", "barrier_fallbacks", "persistent_reason")}


def _vectors(S, names=VECS):
    return {k: S.get(k, S.n if k.startswith("x") or k == "dual_slack" else S.m) for k in names}


# ---- 1. blocks of steps against the oracle ----------------------------------------------------------------------------
@pytest.mark.parametrize("name,steps", [("afiro", 2), ("afiro", 40), ("adlittle", 7), ("25fv47", 40), ("shell", 40)])
def test_persistent_steps_bit_exact(name, steps, monkeypatch):
    """stage("steps_persistent", init=[s]): step 1 by the plain launches, the steps 2..s in ONE persistent launch, the last
    one major — x, y, x_next, y_next are the oracle's bits, and those of stage("steps") on a solver with the switch off.
    afiro is one work block per operand (no cross-workgroup traffic), s = 2 is a launch of one step which is the major one,
    25fv47 is 21 workgroups in the XCD-local mode, shell 8."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    lp, ref = _lp(name), _probe(name, steps)
    monkeypatch.setenv(SWITCH, "1")
    S = solver.DeviceSolver(lp=lp, solver="hipdlp")
    assert _counters(S) == dict(persistent_launches=0, step_barriers=2, barrier_fallbacks=0, persistent_reason=0)
    assert _stage(S, "persistent_mode") == 1
    S.set("steps", [ref["tau"], ref["sigma"]])
    S.stage("steps_persistent", init=[steps])
    got = _vectors(S)
    assert _counters(S) == dict(persistent_launches=1, step_barriers=2, barrier_fallbacks=0, persistent_reason=0)
    S.close()
    for k, r in zip(VECS, ("x_cur", "y_cur", "x_next", "y_next")):
        assert np.array_equal(got[k], ref[r]), k
    monkeypatch.setenv(SWITCH, "0")
    P = solver.DeviceSolver(lp=lp, solver="hipdlp")
    assert _counters(P) == dict(persistent_launches=0, step_barriers=0, barrier_fallbacks=0, persistent_reason=1)
    P.set("steps", [ref["tau"], ref["sigma"]])
    P.stage("steps", init=[steps])
    plain = _vectors(P)
    with pytest.raises(RuntimeError):  # a solver that keeps the plain launches never runs them under this name
        P.stage("steps_persistent", init=[steps])
    P.close()
    for k in VECS:
        assert np.array_equal(got[k], plain[k]), k


# ---- 2. whole solves, switch on against off ---------------------------------------------------------------------------
# Iteration caps chosen on the CPU with O.hipdlp_solve_fn() at kkt_tolerance 1e-4 so that restarts fall inside the run
# (iterations / restarts there: afiro converges after 280 / 6, adlittle after 1280 / 7, shell after 4800 / 15; 25fv47 and
# 80bau3b reach a cap of 400 with 4 restarts).  A restart moves the anchors between two launches and sets the Halpern
# counter back to zero: the case the launch's epoch numbering must survive.
CAPS = {"afiro": 2000, "adlittle": 2000, "25fv47": 800, "shell": 6000, "80bau3b": 400}
RESULT_SCALARS = ("num_iter", "num_restarts", "term_code", "primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap",
                  "norm_rhs", "norm_cost")


def _solve(name, monkeypatch, switch, options=None):
    monkeypatch.setenv(SWITCH, switch)
    opts = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=CAPS[name]) if options is None else options
    S = solver.DeviceSolver(lp=_lp(name), solver="hipdlp", **opts)
    out = S.solve()
    c = _counters(S)
    c["mode"] = int(_stage(S, "persistent_mode"))
    S.close()
    return out, c


def _same_result(a, b):
    for k in ("col_value", "col_dual", "row_value", "row_dual"):
        assert np.array_equal(getattr(a.solution, k), getattr(b.solution, k)), k
    for k in RESULT_SCALARS:
        assert getattr(a.result, k) == getattr(b.result, k), k
    assert a.model_status == b.model_status and a.pdlp_iteration_count == b.pdlp_iteration_count


@pytest.mark.parametrize("name", ["afiro", "adlittle", "25fv47", "shell"])
def test_whole_solve_same_bits_switch_on_and_off(name, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    off, c_off = _solve(name, monkeypatch, "0")
    on, c_on = _solve(name, monkeypatch, "1")
    assert off.result.num_restarts >= 1
    assert c_off["persistent_launches"] == 0 and c_off["step_barriers"] == 0 and c_off["persistent_reason"] == 1
    assert c_on["persistent_launches"] > 0 and c_on["step_barriers"] == 2 and c_on["barrier_fallbacks"] == 0 and c_on["mode"] == 1
    _same_result(on, off)


def test_iteration_limit_semantics_with_the_persistent_launch(monkeypatch):
    """pdlp_iteration_limit=200 on adlittle: 200 iterations and the zero start, as the plain path (pdhg.cc:866-877)."""
    on, c = _solve("adlittle", monkeypatch, "1", dict(pdlp_iteration_limit=200))
    assert c["persistent_launches"] > 0 and c["barrier_fallbacks"] == 0
    assert on.model_status == solver.kIterationLimit and on.pdlp_iteration_count == 200
    assert not on.solution.col_value.any()


# ---- 3. agent-scope mode ----------------------------------------------------------------------------------------------
def test_agent_scope_mode_by_switch(monkeypatch):
    """25fv47 with the XCD-local mode switched off: the same launch with agent-scope accesses on all XCDs."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    off, _ = _solve("25fv47", monkeypatch, "0")
    monkeypatch.setenv("PDLP_MI355X_XCD_LOCAL", "0")
    on, c = _solve("25fv47", monkeypatch, "1")
    assert c["persistent_launches"] > 0 and c["step_barriers"] == 2 and c["barrier_fallbacks"] == 0 and c["mode"] == 0
    assert off.result.num_restarts >= 1
    _same_result(on, off)


def test_agent_scope_mode_by_size_80bau3b(monkeypatch):
    """80bau3b: 42 work blocks of 512 entries in A and in A', no long major (asserted on what the solver holds) — beyond the
    32 workgroups of the XCD-local mode, within the 64 of the flat barrier."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    monkeypatch.setenv(SWITCH, "1")
    S = solver.DeviceSolver(lp=_lp("80bau3b"), solver="hipdlp")
    for which in (0, 1):
        D = S.device_matrix(which)
        assert D["use_slab"] == 0 and D["chunk"] == 512 and D["n_tasks"] == 0 and D["n_long"] == 0
        assert 33 <= D["n_blocks"] <= 64, D["n_blocks"]
    assert _stage(S, "persistent_mode") == 0 and _stage(S, "persistent_reason") == 0
    S.close()
    off, _ = _solve("80bau3b", monkeypatch, "0")
    on, c = _solve("80bau3b", monkeypatch, "1")
    assert c["persistent_launches"] > 0 and c["step_barriers"] == 2 and c["barrier_fallbacks"] == 0 and c["mode"] == 0
    assert off.result.num_restarts >= 1
    _same_result(on, off)


# ---- 4. host-driven loop ----------------------------------------------------------------------------------------------
def test_host_driven_loop(monkeypatch):
    """PDLP_MI355X_DEVICE_CHECK=0: the host decides between blocks, the steps 2..40 replay from the block's own graph."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    monkeypatch.setenv("PDLP_MI355X_DEVICE_CHECK", "0")
    off, c_off = _solve("25fv47", monkeypatch, "0")
    on, c_on = _solve("25fv47", monkeypatch, "1")
    assert c_off["persistent_launches"] == 0
    assert c_on["persistent_launches"] > 0 and c_on["step_barriers"] == 2 and c_on["barrier_fallbacks"] == 0
    assert off.result.num_restarts >= 1
    _same_result(on, off)


# ---- 5. LPs that do not qualify -----------------------------------------------------------------------------------------
def _first_block_equals(S, ref):
    S.set("steps", [ref["tau"], ref["sigma"]])
    S.stage("steps", init=[40])
    got = _vectors(S)
    for k, r in zip(VECS, ("x_cur", "y_cur", "x_next", "y_next")):
        assert np.array_equal(got[k], ref[r]), k
    c = _counters(S)
    assert c["persistent_launches"] == 0 and c["step_barriers"] == 0 and c["barrier_fallbacks"] == 0
    return c["persistent_reason"]


def test_long_major_keeps_plain_launches(monkeypatch):
    """standgub has rows longer than a 512-entry work block: their segment tasks stay with the plain launches (reason 6)."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    monkeypatch.setenv(SWITCH, "1")
    S = solver.DeviceSolver(lp=_lp("standgub"), solver="hipdlp")
    assert _first_block_equals(S, _probe("standgub", 40, "csr")) == 6
    S.close()


def test_more_than_64_blocks_keeps_plain_launches(monkeypatch):
    """The 20k x 20k synthetic LP of test_large_synthetic_block_bit_exact_and_runs: 313 work blocks (reason 7)."""
    monkeypatch.setenv(SWITCH, "1")
    sp_ = solver.SyntheticProblem(20000, 20000, 160000, 3)
    ref = O.hipdlp_probe(sp_.to_lp(), 40)
    S = solver.DeviceSolver(problem_struct=sp_.struct, solver="hipdlp")
    assert _first_block_equals(S, ref) == 7
    S.close()


def test_slab_layout_keeps_plain_launches(monkeypatch):
    """PDLP_MI355X_SLAB=1 (25fv47: the slab layout's long rows are summed as segment tasks, the oracle follows in its
    device order): reason 4."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "1")
    monkeypatch.setenv(SWITCH, "1")
    S = solver.DeviceSolver(lp=_lp("25fv47"), solver="hipdlp")
    assert _first_block_equals(S, _probe("25fv47", 40, "slab")) == 4
    S.close()


# ---- 6. the fall-back -------------------------------------------------------------------------------------------------
STATE = VECS + ("x_anchor", "y_anchor", "x_reflected", "y_reflected", "dual_slack")


def _run_in_two_legs(monkeypatch, stall):
    """25fv47, fixed-work loop: 80 iterations, [the next persistent launch reports stall code `stall` and does nothing,] 320
    more.  -> (state vectors, the scalars of get("steps"), checks and restarts of the second leg, counters after the first
    leg, after the second leg and after 80 further iterations)."""
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")
    monkeypatch.setenv(SWITCH, "1")
    S = solver.DeviceSolver(lp=_lp("25fv47"), solver="hipdlp")
    st = S.iterate(80)
    assert st.iters == 80
    c0 = _counters(S)
    if stall:
        S.stage("stall_next_block", init=[stall])
    st = S.iterate(320)
    assert st.iters == 320
    c1 = dict(_counters(S), mode=int(_stage(S, "persistent_mode")))
    vec, scal = _vectors(S, STATE), S.get("steps", 8)
    S.iterate(80)
    c2 = _counters(S)
    S.close()
    return vec, scal, (st.checks, st.restarts), c0, c1, c2


@functools.lru_cache(maxsize=None)
def _undisturbed():
    mp = pytest.MonkeyPatch()
    try:
        return _run_in_two_legs(mp, 0)
    finally:
        mp.undo()


@pytest.mark.parametrize("stall", [3, 2])
def test_fall_back_continues_with_the_same_bits(stall, monkeypatch):
    """A failed roll call (3) sends the solver to the plain launches for good, a failed placement check (2) to the agent-scope
    mode; either way the stalled unit's steps 2..40 and its check run again from the unchanged state, and the run ends with
    the bits of the undisturbed one."""
    vec0, scal0, cnt0, a0, a1, a2 = _undisturbed()
    assert a0["persistent_launches"] > 0 and a1["persistent_launches"] > a0["persistent_launches"] and a1["barrier_fallbacks"] == 0
    assert cnt0[1] >= 1  # restarts inside the second leg
    vec, scal, cnt, c0, c1, c2 = _run_in_two_legs(monkeypatch, stall)
    assert c0 == a0
    assert c1["barrier_fallbacks"] == 1 and c2["barrier_fallbacks"] == 1
    if stall == 3:
        assert c1["step_barriers"] == 0 and c1["persistent_reason"] == 8 and c1["mode"] == -1
        assert c2["persistent_launches"] == c1["persistent_launches"]  # stops growing
    else:
        assert c1["step_barriers"] == 2 and c1["persistent_reason"] == 0 and c1["mode"] == 0
        assert c2["persistent_launches"] > c1["persistent_launches"]
    assert cnt == cnt0
    assert np.array_equal(scal, scal0)
    for k in STATE:
        assert np.array_equal(vec[k], vec0[k]), k
