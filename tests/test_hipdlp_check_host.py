"""What tests/test_gpu_hipdlp_check.py relies on, shown without a GPU on tests/hipdlp_check_cases.py alone: every planted
situation reaches the branch of the restated decision its name claims, with the threshold situations exactly on their
threshold and one ulp (one iteration) beside it; every branch class of the statistics is populated at every size from 255 x 257
up; integer data keep every sum exact in any order; and the restated decision, fed the oracle's own per-check sums, predicts
the restarts, primal weights and step sizes of whole oracle solves with ==."""
import math
import os

import numpy as np
import pytest

import hipdlp_check_cases as H
import oraclelib as O
from highs_amd import lp as L

BIG = [s for s in H.SIZES if s != (1, 1)] + [H.KINDS]


def _planned(size, values, square=False, seed=21):
    F = H.formulated(size, values)
    v = H.plan(F, values, np.random.default_rng(seed))
    f = H.square_fpe(F, v, H.BASE["eta"]) if square else None
    return F, v, f


def _products(F, v):
    return H.exact_products(F, v)


def _stats(F, v, prod, unit=None):
    ref = H.reference(v, prod, F.n_eqs, False, unit)
    return np.array([q.fsum for q in ref["q"]] + [0.0, 0.0]), ref


# ---- the situations -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("name", list(H.SITUATIONS))
def test_every_situation_reaches_its_branch(name, values):
    sit = H.SITUATIONS[name]
    if sit.integer_only and values == "real":
        return
    F, v, f = _planned((255, 257), values, square=(values == "integer"))
    prod = _products(F, v)
    if sit.tweak:
        sit.tweak(v, prod)
    stats, _ = _stats(F, v, prod, 1.0 if values == "integer" and name not in ("pid_primal_large", "pid_dual_large", "pid_ratio_high", "pid_ratio_low") else None)
    fpe = H.fixed_point_error(H.BASE["omega"], H.BASE["eta"], stats[0:3])
    if values == "integer":
        assert fpe == f and f == int(f) and f > 1  # a perfect square under the root: an integer, whatever the order of the sums
    state = H.situation_state(name, fpe)
    taken = []
    after, rec = H.decide(state, stats, 0.0, F.norm_rhs, F.norm_cost, taken)
    for b in sit.branches:
        assert b in taken, (name, values, taken)
    if name == "halted":
        assert rec is None and after == state
        return
    assert after["iters"] == state["iters"] + 40 and after["nChecks"] == state["nChecks"] + 1 and rec["iters"] == after["iters"]
    restarted = any(b in taken for b in ("first", "sufficient", "necessary", "artificial"))
    assert rec["restarted"] == after["doRestart"] == after["fpe0Pending"] == (1 if restarted else 0)
    assert after["runFpe0"] == (1 if restarted and not after["halted"] else 0)
    assert after["hIter"] == (0 if restarted else state["hIter"] + 40)
    if "converged_terminate" not in taken:  # (a converged check ends the solve in front of the restart rule)
        assert after["lastTrialFpe"] == (H.INF if restarted else fpe)
    assert after["nRestarts"] == state["nRestarts"] + (1 if restarted else 0)
    if "converged_terminate" in taken:
        assert (after["converged"], after["halted"], after["run"], after["termStatus"], rec["converged"]) == (1, 1, 0, 0, 1)
        assert not restarted and after["lastTrialFpe"] == state["lastTrialFpe"]
    if "limit" in taken:
        assert (after["halted"], after["run"], after["converged"]) == (1, 0, 0) and after["termStatus"] == (1 if state["terminate"] else -1)
    if any(b.startswith("pid_refused") for b in taken):
        assert (after["primalWeight"], after["errSum"], after["lastErr"]) == (state["bestPrimalWeight"], 0.0, 0.0)
    if "pid_taken" in taken:
        assert after["primalWeight"] != state["primalWeight"] and after["lastErr"] != state["lastErr"]
        assert math.isclose(after["tau"] * after["sigma"], state["tau"] * state["sigma"], rel_tol=1e-14)
        assert math.isclose(after["sigma"] / after["tau"], after["primalWeight"] ** 2, rel_tol=1e-14) and after["omega"] == abs(after["primalWeight"])
    if "pid_off" in taken or not restarted:
        assert all(after[k] == state[k] for k in ("primalWeight", "tau", "sigma", "omega", "errSum", "lastErr", "bestGap", "bestPrimalWeight"))
    if "best_improved" in taken:
        assert after["bestGap"] < state["bestGap"] and after["bestPrimalWeight"] == after["primalWeight"]
    if "best_kept" in taken:
        assert after["bestGap"] == state["bestGap"] and after["bestPrimalWeight"] == state["bestPrimalWeight"]
    if "fpe0" in taken:
        assert after["initialFpe"] == fpe != state["initialFpe"]
    else:
        assert after["initialFpe"] == state["initialFpe"]


def test_threshold_situations_sit_on_their_thresholds():
    """The planted numbers meet the thresholds in floating point exactly as the names say: <= against <, > against >=."""
    F, v, f = _planned((255, 257), "integer", square=True)
    s = {k: H.situation_state(k, f) for k in H.SITUATIONS}
    assert 0.2 * s["sufficient_on"]["initialFpe"] == f
    assert 0.2 * s["sufficient_past"]["initialFpe"] < f < 0.2 * s["sufficient_before"]["initialFpe"]
    assert 0.8 * s["necessary_on"]["initialFpe"] == f and 0.2 * s["necessary_on"]["initialFpe"] < f
    assert 0.8 * s["necessary_past"]["initialFpe"] < f < 0.8 * s["necessary_before"]["initialFpe"]
    assert s["last_trial_on"]["lastTrialFpe"] == f and s["last_trial_below"]["lastTrialFpe"] == math.nextafter(f, 0.0)
    on, below = s["artificial_on"], s["artificial_below"]
    assert float(on["hIter"] + 40) == 0.36 * float(on["iters"] + 40) and below["hIter"] + 1 == on["hIter"]


# ---- the statistics' branch classes and exactness ---------------------------------------------------------------------------------
@pytest.mark.parametrize("values", ["integer", "real"])
@pytest.mark.parametrize("size", BIG, ids=H.case_name)
def test_every_branch_class_is_populated(size, values):
    F, v, _ = _planned(size, values)
    if size != H.KINDS:
        assert (F.n, F.m) == size and F.n_eqs == size[1] // 2  # the formulation is the identity on these
    else:
        assert (F.n, F.m, F.n_eqs) == (255, 257, 52 + 51 + 51)
    prod = _products(F, v) if values == "integer" else dict(ax=F.A @ v["x_next"], aty0=F.A.T @ v["y"])
    for name, mask in H.branch_classes(v, prod, F.n_eqs).items():
        if values == "real" and "= 0" in name and "cached" not in name:
            continue  # (zero up to the rounding of the product: the GPU test plants these from the device's own product)
        assert mask.any(), (H.case_name(size), values, name)
    assert v["x_next"][H.COL0] == 0.0 and v["y_next"][H.ROW0] == 0.0 and F.n_eqs > H.ROW0


@pytest.mark.parametrize("size", list(H.SIZES) + [H.KINDS], ids=H.case_name)
def test_integer_data_keep_every_sum_exact(size):
    F, v, _ = _planned(size, "integer")
    assert np.array_equal(F.A.data, np.rint(F.A.data)) and np.abs(F.A.data).max() <= 8 and not np.any(F.col_scale != 1.0)
    prod = _products(F, v)
    ref = H.reference(v, prod, F.n_eqs, False, unit=1.0)
    ini = H.reference_initial(v, dict(ax=prod["ax0"], aty=prod["aty0"]), F.n_eqs, False, unit=1.0)
    for q in ref["q"] + ini["q"]:
        assert q.exact == q.fsum == float(int(q.exact)) and q.abs_sum < 2.0**53
    if min(F.n, F.m) > 1:
        assert all(q.abs_sum > 0 for q in ref["q"])
    scales = H.pow2_scales(F, np.random.default_rng(22))
    sc = H.reference(dict(v, **scales), prod, F.n_eqs, True, unit=2.0**-12)
    assert sc["q"][3].exact != ref["q"][3].exact or F.m == 1
    assert sc["q"][5].exact != ref["q"][5].exact or F.n == 1


def test_the_reference_by_hand():
    """Two columns, two rows, by hand: A = [[1, 2], [0, 3]], row 0 an equality, row 1 an inequality."""
    v = dict(x_next=np.array([1.0, -2.0]), x_reflected=np.array([0.0, 1.0]), y_next=np.array([2.0, 1.0]), y_reflected=np.array([2.0, 3.0]),
             x_anchor=np.array([1.0, 1.0]), y_anchor=np.array([0.0, 0.0]), dual_slack=np.array([-4.0, 5.0]), cost=np.array([1.0, 2.0]),
             rhs=np.array([-5.0, -1.0]), lower=np.array([-H.INF, 1.0]), upper=np.array([2.0, H.INF]))
    A = np.array([[1.0, 2.0], [0.0, 3.0]])
    dy = v["y_next"] - v["y_reflected"]
    prod = dict(ax=A @ v["x_next"], aty=A.T @ v["y_next"], atd=A.T @ dy)
    q = [t.fsum for t in H.reference(v, prod, 1, False, unit=1.0)["q"]]
    # dx = (1, -3), dy = (0, -2), A'dy = (0, -6); ax = (-3, -6): residuals 2 (equality), min(0, -5); aty = (2, 7): c - aty = (-1, -5)
    # s+ = (0, 5), s- = (4, 0): residual (-1 - 0 + 4, -5 - 5 + 0) = (3, -10)
    assert q == [4.0, 10.0, 18.0, 4.0 + 25.0, -10.0 - 1.0, 9.0 + 100.0, 1.0 - 4.0, 5.0, 8.0, 4.0, 10.0, 18.0, 9.0, 5.0]
    r, conv = H.residuals(q + [0.0, 0.0], 1.5, 3.0, 4.0, 1e-4)
    assert (r["pFeas"], r["pObj"], r["dObj"], r["gap"], conv) == (math.sqrt(29.0), -1.5, 1.5 - 11.0 + 5.0 - 8.0, 11.0, False)
    assert H.fixed_point_error(2.0, 0.25, q[0:3]) == math.sqrt(10.0 * 2.0 + 4.0 / 2.0 + 2.0 * 0.25 * 18.0)
    ini = H.reference_initial(dict(v, x=v["x_next"], y=v["y_next"]), dict(ax=prod["ax"], aty=prod["aty"]), 1, False, unit=1.0)
    # derived slack: column 0 has an upper bound only: min(0, -1) = -1; column 1 a lower bound only: max(0, -5) = 0
    assert np.array_equal(ini["slack_pos"], [0.0, 0.0]) and np.array_equal(ini["slack_neg"], [1.0, 0.0])
    assert [t.fsum for t in ini["q"]] == [29.0, -11.0, 0.0 + 25.0, -3.0, 0.0, 2.0]


# ---- the decision against whole oracle solves --------------------------------------------------------------------------------------
def _instance(name):
    return L.HighsLp.from_npz(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "instances", name + ".npz"))


@pytest.mark.parametrize("name,cap", [("afiro", 2000), ("adlittle", 2000), ("25fv47", 800)])
def test_decide_predicts_the_oracle_solve(name, cap):
    """hipdlp_oracle_solve in device-order mode reports, for every check, the sums it decided on: the restatement, started
    from the oracle's initial state and fed those sums, reproduces every restart, primal weight and step size with ==."""
    lp = _instance(name)
    res, recs = O.hipdlp_solve_traced(lp, kkt_tolerance=1e-4, pdlp_iteration_limit=cap)
    prep = O.hipdlp_prepared(lp)
    first, checks = recs[0], recs[1:]
    assert first["iters"] == 0 and len(checks) == res.struct.num_iter // 40 and res.struct.num_restarts >= 4
    s = dict(H.BASE, tau=first["tau"], sigma=first["sigma"], eta=first["eta"], omega=first["omega"], primalWeight=first["primal_weight"],
             bestPrimalWeight=first["primal_weight"], errSum=0.0, lastErr=0.0, fpe=0.0, initialFpe=0.0, tol=1e-4, iters=0, iterLimit=cap,
             hIter=0, nRestarts=0, nChecks=1)
    branches = set()
    for r in checks:
        taken = []
        s, rec = H.decide(s, r["stat"], lp.offset, prep["norm_rhs"], prep["norm_cost"], taken)
        branches.update(t.split(":")[0] for t in taken)
        assert (rec["iters"], rec["restarted"], s["nRestarts"]) == (r["iters"], r["restarted"], r["restarts"]), (name, r["iters"], taken)
        for k, want in (("primalWeight", r["primal_weight"]), ("tau", r["tau"]), ("sigma", r["sigma"]), ("omega", r["omega"]),
                        ("fpe", r["fpe"]), ("initialFpe", r["initial_fpe"])):
            assert s[k] == want, (name, r["iters"], k, s[k], want, taken)
    assert s["halted"] == 1 and s["termStatus"] == (0 if res.struct.term_code == 0 else 1)
    assert s["nRestarts"] == res.struct.num_restarts and {"first", "pid_taken"} <= branches, branches
    print(name, "checks", len(checks), "restarts", s["nRestarts"], "branches", sorted(branches))
