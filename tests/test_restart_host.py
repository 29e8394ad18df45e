"""What tests/test_gpu_restart.py relies on, shown without a GPU on tests/restart_cases.py alone: every planted situation
reaches the branch of the restated decision its name claims (decide is instrumented: it reports the branch it took), with
the margins the situation promises; integer data keep the two squared distances exact integers and the logarithm of the
primal-weight update small; and the restated decision predicts the restarts of the oracle.

The oracle's trace (pdlp_oracle_solve_traced) is written at every check BEFORE the restart, with the beta the decision reads
and the feasibilities and objectives of both iterates it reads (the gap is primal_obj - dual_obj, as the check computes it), so
the comparison is possible: the checks at which `decide` restarts must be exactly those behind which the next record's beta
has other bits (the last record has no successor: a solve ends in front of the restart).  A restart whose beta keeps its bits
(one of the two distances below 1e-10, cupdlp_step.c:166) would be invisible to this: none occurs on the three instances, which
is asserted through the oracle's own count of restarts."""
import math
import os

import numpy as np
import pytest

import check_cases as K
import oraclelib as O
import restart_cases as R
from highs_amd import lp as L
from highs_amd import solver

_prepared = {}
THREE = ("artificial_avg", "artificial_cur", "sufficient")
CASES = [((255, 257), s) for s in R.SITUATIONS] + [(size, s) for size in K.SIZES if size != (255, 257) for s in THREE]
DECAY = ("sufficient", "not_sufficient_not_necessary", "necessary", "too_slow", "artificial_edge_25", "artificial_edge_26")


def _form(n, m, values):
    key = (n, m, values)
    if key not in _prepared:
        _prepared[key] = solver.Prepared(K.sized_lp(n, m, values), **(dict(pdlp_features_off=1) if values == "integer" else {}))
    return _prepared[key]


def _plan(size, situation, values, beta):
    P = _form(*size, values)
    data = dict(cost=P.cost, rhs=P.rhs, lower=P.lower, upper=P.upper)
    scales = (P.row_scale, P.col_scale) if values == "real" else None
    vec, memory, der = R.plan(data, situation, values, np.random.default_rng(31), beta, R.matrix_of(P), P.n_eqs, scales)
    return P, vec, memory, der


@pytest.mark.parametrize("beta", [1.0, 0.01, 100.0])
@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("size,situation", CASES)
def test_every_situation_reaches_its_branch(size, situation, values, beta):
    s = R.SITUATIONS[situation]
    P, vec, memory, der = _plan(size, situation, values, beta)
    taken = []
    kind, after = R.decide(der[:10], der[10:], beta, s.it, memory, taken)
    branch, mu = taken[0]
    assert (branch, kind) == (s.branch, s.kind), (situation, branch, kind, mu)
    cur = tuple(der[k] for k in (R.PFEAS, R.DFEAS, R.GAP))
    avg = tuple(der[10 + k] for k in (R.PFEAS, R.DFEAS, R.GAP))
    cand = cur if s.near == "cur" else avg
    lr_before, lr_after = tuple(memory[1:4]), tuple(after[1:4])
    if branch == "first":
        assert lr_after == cur and tuple(after[4:7]) == cur
        return
    assert max(mu["muCur"], mu["muAvg"]) >= 10.0 * min(mu["muCur"], mu["muAvg"]), (situation, mu)  # decided by orders of magnitude
    assert (mu["muCur"] < mu["muAvg"]) == (s.near == "cur")
    assert tuple(after[4:7]) == cand  # LC moves in every branch that computed a candidate
    assert lr_after == (cand if kind else lr_before)  # LR only on a restart
    assert after.iLast == memory.iLast  # (finish moves it)
    if situation in DECAY:  # the margins are the situation's, far above any summation order's effect on a score
        length = max(P.n, P.m)
        assert (length + 1) * 2.0**-53 < 1e-6 * R.MARGIN
        c, lr = mu["muCand"], R.score(beta, *memory[1:4])  # (the artificial branch itself does not compute muLR)
        want = {"sufficient": 0.2 * (1 - R.MARGIN), "not_sufficient_not_necessary": 0.2 * (1 + R.MARGIN), "necessary": 0.8 * (1 - R.MARGIN)}
        assert math.isclose(c / lr, want.get(situation, 0.8 * (1 + R.MARGIN)), rel_tol=1e-12), (situation, c / lr)
        if situation != "sufficient":
            assert math.isclose(R.score(beta, *memory[4:7]) / c, 1 + R.MARGIN if situation == "not_sufficient_not_necessary" else 1 - R.MARGIN, rel_tol=1e-12)
        if situation.startswith("artificial_edge"):
            assert (s.it - s.iLast >= 0.36 * s.it) == (situation == "artificial_edge_25") and s.it - s.iLast in (14, 15)


@pytest.mark.parametrize("size,situation", CASES)
def test_integer_data_keep_the_distances_exact(size, situation):
    s = R.SITUATIONS[situation]
    if s.kind == 0:
        return
    P, vec, memory, der = _plan(size, situation, "integer", 1.0)
    v = dict(vec, x_avg=vec["x_sum"], y_avg=vec["y_sum"], ax_avg=R.matrix_of(P) @ vec["x_sum"], aty_avg=R.matrix_of(P).T @ vec["y_sum"])
    want = R.expected_vectors(v, vec["x_last"], vec["y_last"], s.kind, integer=True)
    for q in (want["dP2"], want["dD2"]):
        assert isinstance(q.exact, int) and 0 <= q.exact < 2**53 and q.abs_sum < 2.0**53 and q.fsum == float(q.exact)
    assert (want["dP2"].exact == 0) == (situation == "still") or min(size) == 1
    if situation == "nearly_still":
        assert want["dP2"].exact == 1
        real = _plan(size, situation, "real", 1.0)[1]
        assert 1e-10 < abs(real["x"] - real["x_last"]).sum() == np.linalg.norm(real["x"] - real["x_last"]) < 0.1
    for beta in (1.0, 0.37, 40.0):
        lg = R.log_beta_update(beta, want["dP2"].exact, want["dD2"].exact)
        assert lg is None or abs(lg) <= 8.0, (situation, lg)
    assert R.same_bits(want["x_last"], vec["x_sum"] if s.kind == 2 else vec["x"]) and not np.any(want["x_sum"]) and not np.any(want["y_sum"])


def test_finish_by_hand():
    """beta = 4, steps 1 and 4 (mean 2), distances 3 and 12: log(12 / 3) / 2 + log(2) / 2 = log(2) + log(2) / 2, beta' = 8 up to
    the roundings of exp and log; primalStep' = 2 / sqrt(beta'), dualStep' = primalStep' beta'."""
    state = dict(tau=9.0, sigma=9.0, beta=4.0, eta=9.0, primalStep=1.0, dualStep=4.0, sumPrimalStep=3.0, sumDualStep=5.0, iLast=0, nRestarts=2)
    out = R.finish(state, 2, 9.0, 144.0, True, 40)
    assert math.isclose(out["beta"], 8.0, rel_tol=1e-14) and math.isclose(out["primalStep"], 2 / math.sqrt(8.0), rel_tol=1e-14)
    assert out["dualStep"] == out["primalStep"] * out["beta"] and out["eta"] == math.sqrt(out["primalStep"] * out["dualStep"])
    assert (out["sumPrimalStep"], out["sumDualStep"], out["iLast"], out["nRestarts"]) == (0.0, 0.0, 40, 3)
    assert math.isclose(out["tau"] * out["sigma"], out["eta"] ** 2, rel_tol=1e-14) and math.isclose(out["sigma"] / out["tau"], out["beta"], rel_tol=1e-14)
    still = R.finish(state, 1, 0.0, 144.0, False, 40)  # dP = 0: beta keeps its bits, the steps are re-derived from it
    assert still["beta"] == 4.0 and (still["primalStep"], still["dualStep"]) == (1.0, 4.0) and (still["tau"], still["sigma"]) == (1.0, 4.0)
    assert R.finish(state, 0, 9.0, 144.0, True, 40) == state


def _instance(name):
    if name == "restart_lp":
        return L.special_lps()["restart_lp"]
    return L.HighsLp.from_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances", name + ".npz"))


@pytest.mark.parametrize("name", ["adlittle", "25fv47", "restart_lp"])
def test_decide_predicts_the_oracle_restarts(name):
    recs = []
    res = O.oracle_solve(_instance(name), trace=recs, kkt_tolerance=1e-4)
    assert len(recs) > 3
    memory = R.Memory(0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    predicted, seen = [], []
    for k, r in enumerate(recs[:-1]):
        cur, avg = np.zeros(10), np.zeros(10)
        cur[[R.PFEAS, R.DFEAS, R.GAP]] = r["primal_feas"], r["dual_feas"], r["primal_obj"] - r["dual_obj"]
        avg[[R.PFEAS, R.DFEAS, R.GAP]] = r["primal_feas_avg"], r["dual_feas_avg"], r["primal_obj_avg"] - r["dual_obj_avg"]
        kind, memory = R.decide(cur, avg, r["beta"], r["iter"], memory)
        if kind:
            memory = memory._replace(iLast=r["iter"])
            predicted.append(r["iter"])
        if recs[k + 1]["beta"] != r["beta"]:
            seen.append(r["iter"])
    assert predicted == seen, (name, predicted, seen)
    assert len(predicted) == res.struct.num_restarts > 0, (name, len(predicted), res.struct.num_restarts)
