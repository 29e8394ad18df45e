"""What tests/test_gpu_trial.py relies on, proven without a GPU (tests/trial_cases.py has the restatement):

  a. every situation reaches the branch it names, and the threshold situations sit ON their thresholds, on the exact sums of
     the iterate they plant;
  b. integer data keep every term on one power-of-two grid and every sum below 2^53 grid units, at every case
     (trial_cases.exact_sum asserts it while it sums);
  c. the work-block counts the cases are built for are the host planner's;
  d. the formulation of these problems neither permutes, negates nor adds anything, so the restatement may multiply with the
     LP's own arrays;
  e. the restated decision predicts whole solves of the CPU oracle with `==`: every trial's accept / reject, the eta, tau and
     sigma the next trial starts from, both step sizes and both step sums — on afiro, adlittle, 25fv47 and a small QP with a
     sparse Hessian, from the oracle's per-trial read-out (pdlp_oracle_solve_trials), fed with the oracle's own sums;
  f. the refresh rule of the power table as restated."""
import math
import os

import numpy as np
import pytest

import oraclelib as O
import qp_small_cases as Q
import trial_cases as T
from highs_amd import lp as L
from highs_amd import solver

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_prepared = {}


def _prepared_of(case, qp=None):
    key = (case, qp)
    if key not in _prepared:
        _prepared[key] = solver.Prepared(T.lp_of(case, "integer", qp), **T.options("integer"))
    return _prepared[key]


def _iterate(case, qp, kind, seed=3):
    lp, P = T.lp_of(case, "integer", qp), _prepared_of(case, qp)
    N = T.matrices(lp)[1]
    data = dict(cost=P.cost, rhs=P.rhs, lower=P.lower, upper=P.upper, nx=N is not None)
    v = T.planted_iterate(lp, data, "integer", np.random.default_rng(seed), P.n_eqs, kind)
    v.update(cost=P.cost, rhs=P.rhs, lower=P.lower, upper=P.upper)
    if qp:
        v["qdiag"] = T.dyadic_qdiag(P.n, np.random.default_rng(seed + 1))
    return lp, P, v


# ---- a ------------------------------------------------------------------------------------------------------------------------
def _situations():
    out = []
    for qp in (None, "diag", "sparse"):
        for name in T.ALL_SITUATIONS:
            if (name in T.QP_SITUATIONS and qp != "sparse") or (name in T.LP_ONLY and qp == "sparse"):
                continue
            out.append((name, qp))
    return out


@pytest.mark.parametrize("name,qp", _situations())
def test_situation_is_where_it_claims_to_be(name, qp):
    kind, tau, sigma = T.ALL_SITUATIONS[name][:3]
    lp, P, v = _iterate("255x257", qp, kind)
    nxt, sums = T.restate_trial(lp, v, tau, sigma, P.n_eqs)
    state = T.situation_state(name, sums)
    claims, after = T.claims(name, state, sums)
    assert all(claims.values()), (name, qp, claims, sums)
    assert after["nTrials"] == state["nTrials"] + 1 and after["pending"] == 0
    if after["lastAccepted"]:
        assert after["cur"] == 1 - state["cur"] and after["nIter"] == state["nIter"] + 1 and after["avgW"] == after["avgWx"] == after["eta"]
    else:
        assert after["cur"] == state["cur"] and after["nIter"] == state["nIter"] and after["avgW"] == after["avgWx"] == 0.0
        assert after["sumPrimalStep"] == state["sumPrimalStep"] and after["primalStep"] == state["primalStep"]


def test_situations_cover_every_choice_of_the_decision():
    seen = set()
    for name, qp in _situations():
        kind, tau, sigma = T.ALL_SITUATIONS[name][:3]
        lp, P, v = _iterate("255x257", qp, kind)
        sums = T.restate_trial(lp, v, tau, sigma, P.n_eqs)[1]
        taken = {}
        T.decide(T.situation_state(name, sums), sums["dX2"], sums["dY2"], sums["inter"], sums["qint"], taken)
        seen |= {k for k in ("den_zero", "first_wins", "second_wins", "accepted", "halted") if taken.get(k)}
        seen |= {"rejected"} if not taken["accepted"] else set()
        seen |= {"inter<0"} if sums["inter"] < 0 else {"inter>0"} if sums["inter"] > 0 else {"inter=0"}
        seen |= {"qint<0"} if sums["qint"] < 0 else {"qint>0"} if sums["qint"] > 0 else set()
    assert seen == {"den_zero", "first_wins", "second_wins", "accepted", "rejected", "halted", "inter<0", "inter>0", "inter=0", "qint<0", "qint>0"}


# ---- b, c, d ------------------------------------------------------------------------------------------------------------------
def _n_operand(hess, n):
    return dict(n=n, m=n, nnz=hess["nnz_off"], spmv_blocks_ax=0, spmv_blocks_aty=0,
                **{o + s: hess["q" + s] for o in ("csr", "csc") for s in ("_beg", "_idx", "_val")})


@pytest.mark.parametrize("case,qp", [(c, qp) for c in T.CASES for qp in (None,) + T.CASES[c][1]])
def test_case_is_exact_and_has_the_planners_blocks(case, qp):
    lp, P, v = _iterate(case, qp, "natural")
    # d: the restatement's matrix is the product's
    assert (P.n, P.m) == (lp.num_col, lp.num_row) and np.array_equal(P.csc_beg, lp.a_start)
    assert np.array_equal(P.csc_idx, lp.a_index) and np.array_equal(P.csc_val, lp.a_value) and np.array_equal(P.cost, lp.col_cost)
    assert np.array_equal(P.row_new_idx, np.arange(P.m)) and P.n_eqs == P.m // 2
    # b: (exact_sum asserts the grid and the 2^53 units)
    nxt, sums = T.restate_trial(lp, v, 2.0**-4, 2.0**-5, P.n_eqs)
    assert sums["dX2"] > 0 and sums["dY2"] > 0 and sums["inter"] != 0 and math.isfinite(T.limit_of(sums, 4.0))
    assert (sums["qint"] != 0) == (qp == "sparse")
    # c
    a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
    assert (a["n_blocks"] + a["n_long"], at["n_blocks"] + at["n_long"], a["chunk"], at["chunk"]) == (*T.BLOCKS[case][:2], T.BLOCKS[case][2], T.BLOCKS[case][2])
    assert a["n_long"] == at["n_long"] == 0
    assert (P.nnz >= 2**18) == (T.BLOCKS[case][2] == 2048)
    if qp == "sparse":
        form, hess = solver.host_prepare_qp(lp, **T.options("integer"))
        pn = solver.stream_plan(_n_operand(hess, P.n), 0)
        assert pn["n_long"] == 0 and pn["chunk"] == 512
        if case in ("blocks256", "blocks257"):
            assert pn["n_blocks"] == T.BLOCKS[case][0]  # two entries per row of N: the counts of A and A'
    # the persistent loop's grid, where the operands qualify at all (whether it is resident is the device's to say)
    print(case, qp, "partials", T.BLOCKS[case], "small_grid", a["small_grid"], at["small_grid"])


# ---- e ------------------------------------------------------------------------------------------------------------------------
def _follow(recs, what):
    """Every record against the restated decision of its own inputs, and against the record behind it.  A record carries the
    step sums as they stand BEHIND its trial, so a trial starts from the sums of the record in front of it — unless a check
    iteration restarted in between (sums zeroed: the accepted trial's sums are then its weight alone)."""
    assert len(recs) > 0
    rejected = 0
    for k, r in enumerate(recs):
        prev = recs[k - 1] if k else None
        state = dict(T.BASE, eta=r["eta"], beta=r["beta"], tau=r["tau"], sigma=r["sigma"], nIter=r["iter"], nTrials=r["trials"] - 1,
                     cur=r["iter"] % 2, sumPrimalStep=prev["sum_primal_step"] if prev else 0.0,
                     sumDualStep=prev["sum_dual_step"] if prev else 0.0, powBase=0, powCount=0, commError=0, pending=0)
        after = T.decide(state, r["dx2"], r["dy2"], r["inter"], r["qint"])
        assert after["lastAccepted"] == r["accepted"], (what, k, r)
        assert after["movement"] == r["movement"] and after["limit"] == r["limit"], (what, k, r)
        if r["accepted"]:
            assert (after["primalStep"], after["dualStep"]) == (r["primal_step"], r["dual_step"]), (what, k, r, after)
            if (r["sum_primal_step"], r["sum_dual_step"]) != (after["sumPrimalStep"], after["sumDualStep"]):
                assert prev is not None and (r["iter"] < 10 or r["iter"] % 40 == 0), (what, k, r, after)  # only behind a check iteration
                assert r["sum_primal_step"] == r["sum_dual_step"] == after["avgW"], (what, k, r, after)
        else:
            rejected += 1
            assert after["eta"] == r["eta_out"], (what, k)
            assert (r["sum_primal_step"], r["sum_dual_step"]) == (state["sumPrimalStep"], state["sumDualStep"]) or r["iter"] < 10 or r["iter"] % 40 == 0
        if k + 1 < len(recs):  # what the NEXT trial starts from (a restart in between changes beta, and with it the steps)
            nx = recs[k + 1]
            assert nx["trials"] == r["trials"] + 1 and nx["iter"] == r["iter"] + r["accepted"], (what, k)
            if nx["beta"] == r["beta"]:
                assert (after["eta"], after["tau"], after["sigma"]) == (nx["eta"], nx["tau"], nx["sigma"]), (what, k, r, nx, after)
    return rejected


@pytest.mark.parametrize("name", ["afiro", "adlittle", "25fv47"])
def test_restated_decision_predicts_the_oracles_solve(name):
    lp = L.HighsLp.from_npz(os.path.join(ROOT, "tests", "golden", "instances", name + ".npz"))
    R, recs = O.oracle_solve_trials(lp, kkt_tolerance=1e-4, iter_limit=4000 if name == "25fv47" else 100000)
    plain = O.oracle_solve(lp, kkt_tolerance=1e-4, iter_limit=4000 if name == "25fv47" else 100000)
    assert (R.num_iter, R.num_trials, R.primal_obj) == (plain.num_iter, plain.num_trials, plain.primal_obj)  # the read-out changes nothing
    assert len(recs) == R.num_trials and sum(r["accepted"] for r in recs) == R.num_iter
    rejected = _follow(recs, name)
    print(name, "trials", len(recs), "rejected", rejected)
    assert rejected > 0


def test_restated_decision_predicts_the_oracles_solve_of_a_sparse_qp():
    lp = Q.mpc()
    R, recs = O.oracle_solve_trials(lp, kkt_tolerance=1e-6, iter_limit=20000)
    assert len(recs) == R.num_trials and any(r["qint"] != 0.0 for r in recs)
    rejected = _follow(recs, "mpc")
    print("mpc trials", len(recs), "rejected", rejected, "trials with qint < 0", sum(r["qint"] < 0 for r in recs))


# ---- f ------------------------------------------------------------------------------------------------------------------------
def test_power_table_refresh_rule():
    W, M = T.POW_WINDOW, T.POW_MARGIN
    assert (W, M) == (16384, 4096)
    assert T.pow_table_after_push(0, 0, 0) == (0, W)
    assert T.pow_table_after_push(W - M - 1, 0, W) == (0, W) and T.pow_table_after_push(W - M, 0, W) == (W - M, W)  # 12287 | 12288
    assert T.pow_table_after_push(5, 12288, W) == (5, W) and T.pow_table_after_push(10**6, 0, W) == (10**6, W)
    # behind every push the margin covers the stretches the loop runs without one (160 iterations and their rejected trials)
    for n_trials in (0, 1, 12287, 12288, 10**6):
        base, count = T.pow_table_after_push(n_trials, 0, W)
        assert T.covered(dict(nTrials=n_trials, powBase=base, powCount=count)) and base + count - n_trials > M
