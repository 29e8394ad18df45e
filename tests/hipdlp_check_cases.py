"""Generated problems, planted states, an order-free reference for the 14 sums of a HiPDLP check iteration and a restatement
of the decision taken on them: for tests/test_hipdlp_check_host.py and tests/test_gpu_hipdlp_check.py.  Fixed seeds, nothing
read from disk.

The check iteration of solver="hipdlp" (highs_amd/csrc/pdlp_halpern.cpp enqueueUnitTail, or the same kernels queued by the
host-driven loop) leaves 16 statistics slots:
  0 |dy|^2   1 |dx|^2   2 <dx, A'dy>      dy = y_next - y_reflected, dx = x_next - x_reflected      computeFixedPointError
  3 |rowScale . proj(A x_next - b)|^2 (proj = min(., 0) on inequality rows)   4 b'y_next             computePrimalFeasibility
  5 |colScale . (c - A'y_next - s+ + s-)|^2   6 c'x_next   7 l's+   8 u's-      computeDualFeasibility / computeDualObjective
  9..11 the three sums of slot 0..2 again (behind the first step of a block that follows a restart)
  12 |x_next - x_anchor|^2   13 |y_next - y_anchor|^2                                              updatePrimalWeightAtRestart
  14, 15 unused (zero)
with s+ = max(0, ds), s- = max(0, -ds) and ds the cached dual slack of the last major step, or, in the check of iteration 0
("derived"), c - A'y projected by bound kind.  The reference is written from hipdlp/pdhg.cc of the reference implementation —
computeFixedPointError :709-739, computePrimalFeasibility :1297-1320, computeDualSlacks :1322-1378 (Halpern branch),
computeDualFeasibility :1380-1408, computeDualObjective :1447-1472, checkConvergence :1474-1527, checkRestartCriteria :901-927,
updatePrimalWeightAtRestart :1979-2050 — with numpy on whole vectors, each step in the order of that text; std::max(a, b) and
std::min(a, b) are written as the comparisons they are.  The products A x, A'y and A'dy are inputs: exact integers in integer
mode, read from the device in real mode (where the GPU test holds them to the any-order bound on their own).

The decision (`decide`) restates the block loop :578-707 on the sums the device returned, in float64 scalar arithmetic; its
log / exp are the oracle's plain-arithmetic functions (oraclelib pdlp_oracle_det_exp_log), as the product computes them on the
device, so that every number it derives is comparable with ==."""
import math
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import check_cases as K
import oraclelib as O
from highs_amd import abi
from highs_amd import lp as L

INF = float("inf")
N_SLOTS = 16
STAT_NAMES = ("fpe_dy2", "fpe_dx2", "fpe_cross", "pres2", "by", "dres2", "cx", "l_sp", "u_sn", "fpe0_dy2", "fpe0_dx2", "fpe0_cross",
              "dist_x2", "dist_y2", "unused14", "unused15")
# get / set "halpern_state" (pdlp_halpern.cpp stateToArray): the scalars the decision reads or writes, then StandardForm::scaled
STATE_NAMES = ("tau", "sigma", "eta", "omega", "primalWeight", "bestPrimalWeight", "bestGap", "errSum", "lastErr", "fpe", "initialFpe",
               "lastTrialFpe", "tol", "iters", "iterLimit", "hIter", "pid", "terminate", "nRestarts", "nChecks", "fpe0Pending", "halted",
               "converged", "doRestart", "run", "runFpe0", "termStatus", "scaled")
RECORD_NAMES = ("iters", "pObj", "dObj", "gap", "relGap", "pFeas", "dFeas", "fpe", "primalWeight", "restarted", "converged")
INTERVAL = 40  # PDHG_CHECK_INTERVAL, pdhg.cc:32
ITERATE = ("x", "y", "x_next", "y_next", "x_reflected", "y_reflected", "x_anchor", "y_anchor", "dual_slack")
DATA = ("cost", "rhs", "lower", "upper")
ROW_VECTORS = ("y", "y_next", "y_reflected", "y_anchor", "rhs", "row_scale", "out_y", "check_ax", "delta_y")

Quantity = K.Quantity


# ---- problems -----------------------------------------------------------------------------------------------------------------
# check_cases.SIZES and one more: 255 columns and 524100 rows — the restart and output copies run over n + m flat: the split
# between the column and the row side then lies inside the first block, and the flat index passes 524288 (a second
# grid-stride trip) on the row side
SIZES = K.SIZES + ((255, 524100),)
KINDS = "kinds255x257"  # 153 columns, 257 rows of all five kinds: 102 slack columns, 255 x 257 as the solver holds it
ROW_KINDS = ("eq", "geq", "leq", "ranged", "free")
_made = {}


def kinds_lp(values):
    """Row i has kind i % 5 (equality, >=, <=, ranged, free): the formulation negates the <= rows, gives the ranged and the
    free rows a slack column each and moves them in front of the inequality rows."""
    n0, m = 153, 257
    base = K.stats_lp(n0, m, values, seed=4242)
    rng = np.random.default_rng(4243)
    kind = np.arange(m) % 5
    b = K._values(rng, m, values, lo=0)
    width = np.abs(K._values(rng, m, values)) + (0.0 if values == "integer" else 0.5)
    row_lower = np.where((kind == 2) | (kind == 4), -INF, b)
    row_upper = np.where(kind == 0, b, np.where(kind == 2, b, np.where(kind == 3, b + width, INF)))
    return L.HighsLp(n0, m, base.col_cost, base.col_lower, base.col_upper, row_lower, row_upper, base.a_start, base.a_index,
                     base.a_value, 1, 0.0, "kinds_%s" % values).normalise()


def case_name(size):
    return size if isinstance(size, str) else "%dx%d" % size


def case_lp(size, values):
    """The LP of a case: (n, m) of SIZES -> check_cases.sized_lp; KINDS -> kinds_lp.  Made once."""
    key = (case_name(size), values)
    if key not in _made:
        _made[key] = kinds_lp(values) if size == KINDS else K.sized_lp(size[0], size[1], values)
    return _made[key]


def options(values):
    return dict(solver="hipdlp", pdlp_features_off=1) if values == "integer" else dict(solver="hipdlp")


Form = namedtuple("Form", "n m n_eqs A cost rhs lower upper col_scale row_scale norm_cost norm_rhs row_upper")
_forms = {}


def formulated_lp(lp, values):
    """Any LP as the oracle's own formulation and scaling of this path hold it (hipdlp_oracle_prepare: independent of the
    product's set-up, which other tests compare with it array for array), under options(values)."""
    P = O.hipdlp_prepared(lp, **{k: v for k, v in options(values).items() if k != "solver"})
    A = sp.csc_matrix((P["val"], P["idx"], P["beg"]), shape=(P["m"], P["n"]))
    return Form(P["n"], P["m"], P["n_eqs"], A, P["cost"], P["row_lower"], P["lower"], P["upper"], P["col_scale"],
                P["row_scale"], P["norm_cost"], P["norm_rhs"], P["row_upper"])


def formulated(size, values):
    """formulated_lp of a case of this file.  Made once."""
    key = (case_name(size), values)
    if key not in _forms:
        _forms[key] = formulated_lp(case_lp(size, values), values)
    return _forms[key]


# ---- planted states -----------------------------------------------------------------------------------------------------------
ROW0, COL0 = 0, 0  # an equality row with y_next = 0 and a column with x_next = 0: where a situation plants a huge datum


def _small(rng, k, values):
    return rng.integers(-16, 17, size=k).astype(np.float64) if values == "integer" else rng.standard_normal(k)


def _mag(rng, k, values):
    return rng.integers(1, 101, size=k).astype(np.float64) if values == "integer" else np.abs(rng.standard_normal(k)) + 0.01


def _sign3(k):
    return np.where(k % 3 == 0, -1.0, np.where(k % 3 == 1, 0.0, 1.0))


def row_class(F):
    """Per row: 0 / 1 / 2 = A x_next - b planted negative / zero / positive, cycling within the equality rows and within the
    inequality rows."""
    i = np.arange(F.m)
    return np.where(i < F.n_eqs, i, i - F.n_eqs) % 3


def plan(F, values, rng, lower=None, upper=None):
    """The vectors to plant on a solver of the formulated problem F: the nine iterate vectors, and cost, rhs and bounds.
      rhs    = A x_next - s_i |.|    s_i = -1 / 0 / +1 by row_class: the residual of the cached check, on equality and on
                                     inequality rows (real mode: zero up to the rounding of A x_next; the GPU test sets the
                                     zero class from the device's own product)
      dual_slack_j = s |.|           s by (j // 5) % 3, against the bound kind j % 5 (free, lower, upper, boxed, fixed)
      cost   = A'y + s |.|           s by (j // 5 + 1) % 3: c - A'y of the derived check (iteration 0, on x and y)
      bounds   the problem's own, with -0.0 planted as a finite bound in every seventh group of five columns
    x_next[COL0] = 0 and y_next[ROW0] = 0.  Integer mode: iterates in [-16, 16], magnitudes in [1, 100]."""
    n, m = F.n, F.m
    j = np.arange(n)
    v = {k: _small(rng, m if k in ROW_VECTORS else n, values) for k in ITERATE if k != "dual_slack"}
    v["x_next"][COL0] = 0.0
    v["y_next"][ROW0] = 0.0
    v["dual_slack"] = _sign3(j // 5) * _mag(rng, n, values)
    v["rhs"] = F.A @ v["x_next"] - _sign3(row_class(F)) * _mag(rng, m, values)
    v["cost"] = F.A.T @ v["y"] + _sign3(j // 5 + 1) * _mag(rng, n, values)
    lo, up = (F.lower if lower is None else lower).copy(), (F.upper if upper is None else upper).copy()
    seventh = (j // 5) % 7 == 3
    has_l, has_u = lo > -INF, up < INF
    fixed = has_l & has_u & (lo == up)
    up[seventh & has_l & has_u & ~fixed] = np.maximum(up[seventh & has_l & has_u & ~fixed], 1.0)  # (boxed: -0.0 <= x <= u, u >= 1)
    lo[seventh & has_l] = -0.0
    up[seventh & (fixed | ~has_l) & has_u] = -0.0
    assert np.all(lo <= up)
    v["lower"], v["upper"] = lo, up
    return v


def pow2_scales(F, rng):
    """Power-of-two scale vectors (2^-3 .. 2^3) for the scaled branch of the statistics on integer data."""
    return dict(col_scale=2.0 ** rng.integers(-3, 4, F.n), row_scale=2.0 ** rng.integers(-3, 4, F.m))


def square_fpe(F, v, eta):
    """Integer mode, omega = 1: changes y_reflected on four rows WITHOUT matrix entries (they enter |dy|^2 only) so that
    |dx|^2 + |dy|^2 + 2 eta <dx, A'dy> is a perfect square; returns its root, the fixed-point error."""
    assert 2.0 * eta == int(2.0 * eta)
    empty = np.nonzero(np.diff(F.A.tocsr().indptr) == 0)[0]
    empty = empty[empty != ROW0][-4:]
    assert len(empty) == 4, "the case needs four rows without entries"
    v["y_reflected"][empty] = v["y_next"][empty]
    dx, dy = v["x_next"] - v["x_reflected"], v["y_next"] - v["y_reflected"]
    base = int((dx * dx).sum()) + int((dy * dy).sum()) + int(2.0 * eta) * int((dx * (F.A.T @ dy)).sum())
    assert base >= 0
    root = math.isqrt(base) + 1
    while True:
        rest = root * root - base
        four = _four_squares(rest)
        if four is not None:
            break
        root += 1
    v["y_reflected"][empty] = v["y_next"][empty] - np.array(four, dtype=np.float64)
    return float(root)


def _four_squares(k):
    lim = math.isqrt(k)
    for a in range(lim, -1, -1):
        for b in range(min(a, math.isqrt(k - a * a)), -1, -1):
            r = k - a * a - b * b
            for c in range(min(b, math.isqrt(r)), -1, -1):
                d = math.isqrt(r - c * c)
                if d <= c and c * c + d * d == r:
                    return a, b, c, d
    return None


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _quantity(terms, unit):
    """unit: None (real data), or the power of two every term must be a multiple of — then the sum is exact in any order as
    long as sum|term| / unit stays below 2^53, and `exact` is that sum (fsum rounds the exact sum once: it IS the sum)."""
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    fs, ab = math.fsum(terms), math.fsum(np.abs(terms))
    exact = None
    if unit is not None:
        t = terms / unit
        assert np.array_equal(t, np.rint(t)), "integer data gave a term off the grid"
        assert ab / unit < 2.0**53
        exact = fs
    return Quantity(terms, fs, ab, len(terms), exact)


def _max0(a):  # std::max(0.0, a) = (0.0 < a) ? a : 0.0
    return np.where(0.0 < a, a, 0.0)


def _min0(a):  # std::min(0.0, a) = (a < 0.0) ? a : 0.0
    return np.where(a < 0.0, a, 0.0)


def fpe_terms(v, atd):
    """computeFixedPointError: the terms of its three sums, in the order of the slots (dual, primal, cross)."""
    dx = v["x_next"] - v["x_reflected"]
    dy = v["y_next"] - v["y_reflected"]
    return [dy * dy, dx * dx, dx * atd]


def row_terms(ax, y, b, row_scale, n_eqs, scaled):
    res = ax - b
    res = np.where(np.arange(len(b)) < n_eqs, res, _min0(res))
    if scaled:
        res = res * row_scale
    return [res * res, b * y]


def derived_slack(dr, lower, upper):
    """computeDualSlacks without a cached slack: by bound kind."""
    has_l, has_u = lower > -INF, upper < INF
    return np.where(has_l & has_u, dr, np.where(has_l, _max0(dr), np.where(has_u, _min0(dr), 0.0)))


def col_terms(aty, x, c, lower, upper, col_scale, slack, scaled):
    dr = c - aty
    ds = derived_slack(dr, lower, upper) if slack is None else slack
    s_pos, s_neg = _max0(ds), _max0(-ds)
    res = dr - s_pos + s_neg
    if scaled:
        res = res * col_scale
    l_f, u_f = np.where(lower > -INF, lower, 0.0), np.where(upper < INF, upper, 0.0)
    return [res * res, c * x, np.where(lower > -INF, l_f * s_pos, 0.0), np.where(upper < INF, u_f * s_neg, 0.0)], s_pos + 0.0, s_neg + 0.0


def reference(v, prod, n_eqs, scaled, unit=None):
    """The cached check behind a block: the 14 quantities in slot order (slots 9..11 repeat 0..2) and the two slack vectors,
    from the vectors `v` (as the device holds them) and the products prod = dict(ax = A x_next, aty = A'y_next, atd = A'dy)."""
    f = fpe_terms(v, prod["atd"])
    r = row_terms(prod["ax"], v["y_next"], v["rhs"], v.get("row_scale"), n_eqs, scaled)
    c, s_pos, s_neg = col_terms(prod["aty"], v["x_next"], v["cost"], v["lower"], v["upper"], v.get("col_scale"), v["dual_slack"], scaled)
    dist = [(v["x_next"] - v["x_anchor"]) ** 2, (v["y_next"] - v["y_anchor"]) ** 2]
    return dict(q=[_quantity(t, unit) for t in f + r + c + f + dist], slack_pos=s_pos, slack_neg=s_neg)


def reference_initial(v, prod, n_eqs, scaled, unit=None):
    """The check of iteration 0 on x and y (prod = dict(ax = A x, aty = A'y)): the six quantities of slots 3..8, the slacks."""
    r = row_terms(prod["ax"], v["y"], v["rhs"], v.get("row_scale"), n_eqs, scaled)
    c, s_pos, s_neg = col_terms(prod["aty"], v["x"], v["cost"], v["lower"], v["upper"], v.get("col_scale"), None, scaled)
    return dict(q=[_quantity(t, unit) for t in r + c], slack_pos=s_pos, slack_neg=s_neg)


def exact_products(F, v):
    """Integer mode: the three products of the cached check and the two of the derived one, exact in any order."""
    dy = v["y_next"] - v["y_reflected"]
    out = dict(ax=F.A @ v["x_next"], aty=F.A.T @ v["y_next"], atd=F.A.T @ dy, ax0=F.A @ v["x"], aty0=F.A.T @ v["y"])
    absA = abs(F.A)
    assert max((absA @ np.abs(v["x_next"])).max(), (absA.T @ np.abs(v["y_next"])).max(), (absA.T @ np.abs(dy)).max()) < 2.0**53
    return out


any_order_bound = K.any_order_bound


# ---- which branches a state reaches -------------------------------------------------------------------------------------------
def branch_classes(v, prod, n_eqs):
    """name -> boolean mask: rows by the sign of A x_next - b on equality and on inequality rows; columns by the sign of the
    cached slack, and of c - A'y of the derived check, against the four (has lower, has upper) pairs."""
    i = np.arange(len(v["rhs"]))
    d = prod["ax"] - v["rhs"]
    out = {}
    for name, mask in (("equality", i < n_eqs), ("inequality", i >= n_eqs)):
        out["row %s: ax - b < 0" % name] = mask & (d < 0)
        out["row %s: ax - b = 0" % name] = mask & (d == 0)
        out["row %s: ax - b > 0" % name] = mask & (d > 0)
    has_l, has_u = v["lower"] > -INF, v["upper"] < INF
    dr0 = v["cost"] - prod["aty0"]
    for name, mask in (("free", ~has_l & ~has_u), ("lower", has_l & ~has_u), ("upper", ~has_l & has_u), ("boxed", has_l & has_u)):
        for what, s in (("cached slack", v["dual_slack"]), ("derived c - A'y", dr0)):
            out["col %s: %s < 0" % (name, what)] = mask & (s < 0)
            out["col %s: %s = 0" % (name, what)] = mask & (s == 0)
            out["col %s: %s > 0" % (name, what)] = mask & (s > 0)
    out["col: lower = -0.0"] = (v["lower"] == 0.0) & np.signbit(v["lower"])
    out["col: upper = -0.0"] = (v["upper"] == 0.0) & np.signbit(v["upper"])
    out["col: lower = upper"] = v["lower"] == v["upper"]
    return out


# ---- the decision -------------------------------------------------------------------------------------------------------------
def det_exp_log(x):
    a, e, lg = np.array([float(x)]), np.zeros(1), np.zeros(1)
    O.oracle().pdlp_oracle_det_exp_log(1, a.ctypes.data_as(abi.c_f64p), e.ctypes.data_as(abi.c_f64p), lg.ctypes.data_as(abi.c_f64p))
    return float(e[0]), float(lg[0])


def _log(x):
    return det_exp_log(x)[1]


def _exp(x):
    return det_exp_log(x)[0]


def fixed_point_error(omega, eta, three):
    dual_sq, primal_sq, cross = (float(t) for t in three)
    movement = primal_sq * omega + dual_sq / omega
    interaction = 2.0 * eta * cross
    return math.sqrt(max(0.0, movement + interaction))


def residuals(stats, offset, norm_rhs, norm_cost, tol):
    """checkConvergence on the six sums of slots 3..8 -> (record fields, converged)."""
    s = [float(t) for t in stats]
    r = dict(pFeas=math.sqrt(s[3]), dFeas=math.sqrt(s[5]), pObj=offset + s[6])
    r["dObj"] = ((offset + s[4]) + s[7]) - s[8]
    gap = r["pObj"] - r["dObj"]
    r["gap"] = abs(gap)
    r["relGap"] = abs(gap) / (1.0 + abs(r["pObj"]) + abs(r["dObj"]))
    conv = r["pFeas"] < tol * (1.0 + norm_rhs) and r["dFeas"] < tol * (1.0 + norm_cost) and r["relGap"] < tol
    return r, conv


def update_weight(s, r, dist2, norm_rhs, norm_cost, taken):
    """updatePrimalWeightAtRestart (k_p 0.99, k_i 0.01, k_d 0, i_smooth 0.3) on the state dict s, in place."""
    primal_dist, dual_dist = math.sqrt(float(dist2[0])), math.sqrt(float(dist2[1]))
    rel_primal, rel_dual = r["pFeas"] / (1.0 + norm_rhs), r["dFeas"] / (1.0 + norm_cost)
    ratio = rel_dual / rel_primal if rel_primal > 0.0 else 1e300
    guards = (("primal_small", primal_dist > 1e-16), ("dual_small", dual_dist > 1e-16), ("primal_large", primal_dist < 1e12),
              ("dual_large", dual_dist < 1e12), ("ratio_low", ratio > 1e-8), ("ratio_high", ratio < 1e8))
    if all(ok for _, ok in guards):
        error = _log(dual_dist) - _log(primal_dist) - _log(s["primalWeight"])
        s["errSum"] = 0.3 * s["errSum"] + error
        delta = error - s["lastErr"]
        s["primalWeight"] = s["primalWeight"] * _exp(0.99 * error + 0.01 * s["errSum"] + 0.0 * delta)
        s["lastErr"] = error
        taken.append("pid_taken")
    else:
        s["primalWeight"] = s["bestPrimalWeight"]
        s["errSum"] = 0.0
        s["lastErr"] = 0.0
        taken.append("pid_refused:" + ",".join(name for name, ok in guards if not ok) + ("(relP=0)" if not rel_primal > 0.0 else ""))
    gap = abs(_log(rel_dual / rel_primal) * 0.4342944819032518) if rel_primal > 0.0 and rel_dual > 0.0 else s["bestGap"]
    if gap < s["bestGap"]:
        s["bestGap"] = gap
        s["bestPrimalWeight"] = s["primalWeight"]
        taken.append("best_improved")
    else:
        taken.append("best_kept")
    eta = math.sqrt(s["tau"] * s["sigma"])
    beta = s["primalWeight"] * s["primalWeight"]
    s["tau"] = eta / s["primalWeight"]
    s["sigma"] = eta * s["primalWeight"]
    s["omega"] = math.sqrt(beta)


def decide(state, stats, offset, norm_rhs, norm_cost, taken=None):
    """One check iteration's decision on the 16 sums `stats`: -> (state after, record), both dicts; `taken` collects the
    branches.  A halted state is returned as it is, with no record."""
    taken = [] if taken is None else taken
    s = dict(state)
    if s["halted"]:
        taken.append("halted")
        return s, None
    if s["fpe0Pending"]:
        s["initialFpe"] = fixed_point_error(s["omega"], s["eta"], stats[9:12])
        taken.append("fpe0")
    s["fpe"] = fixed_point_error(s["omega"], s["eta"], stats[0:3])
    s["hIter"] += INTERVAL
    s["iters"] += INTERVAL
    r, conv = residuals(stats, offset, norm_rhs, norm_cost, s["tol"])
    s["nChecks"] += 1
    r.update(iters=s["iters"], fpe=s["fpe"], primalWeight=s["primalWeight"], restarted=0, converged=1 if conv else 0)
    s["doRestart"] = s["runFpe0"] = s["fpe0Pending"] = 0
    if conv and s["terminate"]:
        s.update(converged=1, halted=1, run=0, termStatus=0)
        taken.append("converged_terminate")
        return s, r
    if conv:
        taken.append("converged_ignored")
    restart = False
    if s["iters"] == INTERVAL:
        restart = True
        taken.append("first")
    elif s["iters"] > INTERVAL:
        if s["fpe"] <= 0.2 * s["initialFpe"]:
            restart = True
            taken.append("sufficient")
        elif s["fpe"] <= 0.8 * s["initialFpe"] and s["fpe"] > s["lastTrialFpe"]:
            restart = True
            taken.append("necessary")
        elif float(s["hIter"]) >= 0.36 * float(s["iters"]):
            restart = True
            taken.append("artificial")
    if not restart:
        taken.append("none")
    s["lastTrialFpe"] = s["fpe"]
    if restart:
        if s["pid"]:
            update_weight(s, r, stats[12:14], norm_rhs, norm_cost, taken)
        else:
            taken.append("pid_off")
        s["hIter"] = 0
        s["lastTrialFpe"] = INF
        s["nRestarts"] += 1
        s["doRestart"] = 1
        r["restarted"] = 1
    if s["iters"] >= s["iterLimit"]:
        s["halted"], s["run"] = 1, 0
        if s["terminate"]:
            s["termStatus"] = 1
        taken.append("limit")
    s["fpe0Pending"] = 1 if restart else 0
    s["runFpe0"] = 1 if restart and not s["halted"] else 0
    return s, r


def state_array(state, scaled):
    return np.array([float(state[k]) for k in STATE_NAMES[:-1]] + [1.0 if scaled else 0.0])


def state_dict(arr):
    d = dict(zip(STATE_NAMES, (float(t) for t in arr)))
    for k in STATE_NAMES[13:27]:
        d[k] = int(d[k])
    return d


def record_array(r):
    return np.array([float(r[k]) for k in RECORD_NAMES])


# ---- one Halpern step ---------------------------------------------------------------------------------------------------------
STEP_VECTORS = ("x", "x_next", "x_reflected", "dual_slack", "y", "y_next", "y_reflected")


def _std_min(a, b):  # std::min(a, b) = (b < a) ? b : a
    return np.where(b < a, b, a)


def _std_max(a, b):  # std::max(a, b) = (a < b) ? b : a
    return np.where(a < b, b, a)


def halpern_step(A, d, tau, sigma, h_iter, k_offset, major, rho=1.0):
    """performHalpernPdhgStep, pdhg.cc:961-1018, elementwise in the reference's operation order, on the dict d of vectors (x, y,
    anchors, cost, bounds, rhs, row_upper), in place.  The two products are scipy's: the caller keeps their operands on a
    dyadic grid, so that they are exact in any order."""
    k = h_iter + k_offset
    w = float(k) / (k + 1.0)
    aty = A.T @ d["y"]  # ATy_cache_: A'y_current of the step before
    temp = d["x"] - tau * (d["cost"] - aty)
    proj = _std_max(d["lower"], _std_min(temp, d["upper"]))
    if major:
        d["x_next"] = proj
        d["dual_slack"] = (proj - temp) / tau
    d["x_reflected"] = 2.0 * proj - d["x"]
    ax = A @ d["x_reflected"]
    temp_y = d["y"] / sigma - ax
    proj_y = _std_max(-d["row_upper"], _std_min(temp_y, -d["rhs"]))
    pdhg_dual = (temp_y - proj_y) * sigma
    if major:
        d["y_next"] = pdhg_dual
    d["y_reflected"] = 2.0 * pdhg_dual - d["y"]
    d["x"] = w * (rho * d["x_reflected"] + (1.0 - rho) * d["x"]) + (1.0 - w) * d["x_anchor"]
    d["y"] = w * (rho * d["y_reflected"] + (1.0 - rho) * d["y"]) + (1.0 - w) * d["y_anchor"]
    return temp


def step_plan(F, lower, upper, rng, dyadic_anchors):
    """The start of a step on the integer-matrix problem F: y integer, x and the costs on the grid of 1/4, so that with
    tau = 1/4 the reflected x is on the grid of 1/16 and both products of the step are exact in any order.  Every eleventh
    column with a finite lower (upper) bound starts so that temp = x - tau (c - A'y) lies exactly ON that bound; the bounds are
    plan()'s (five kinds, -0.0, l == u).  Anchors: real, or on the grid of 1/4 (then a second step is exact as well)."""
    n, m = F.n, F.m
    j = np.arange(n)
    d = dict(y=rng.integers(-16, 17, m).astype(np.float64), x=rng.integers(-64, 65, n) / 4.0, cost=F.cost.copy(),
             lower=lower.copy(), upper=upper.copy())
    red = 0.25 * (d["cost"] - F.A.T @ d["y"])
    on_l, on_u = (j % 11 == 0) & (lower > -INF), (j % 11 == 1) & (upper < INF)
    d["x"] = np.where(on_l, lower + red, np.where(on_u, upper + red, d["x"]))
    if dyadic_anchors:
        d["x_anchor"], d["y_anchor"] = rng.integers(-64, 65, n) / 4.0, rng.integers(-64, 65, m) / 4.0
    else:
        d["x_anchor"], d["y_anchor"] = rng.standard_normal(n), rng.standard_normal(m)
    return d


# ---- situations ---------------------------------------------------------------------------------------------------------------
BASE = dict(tau=0.25, sigma=4.0, eta=0.5, omega=1.0, primalWeight=1.0, bestPrimalWeight=3.0, bestGap=INF, errSum=0.125, lastErr=-0.25,
            fpe=7.0, initialFpe=0.0, lastTrialFpe=INF, tol=0.0, iters=400, iterLimit=10**6, hIter=40, pid=1, terminate=1, nRestarts=3,
            nChecks=11, fpe0Pending=0, halted=0, converged=0, doRestart=0, run=1, runFpe0=0, termStatus=-1)
HUGE = 2.0**70
# name -> (mode of the stage, state overrides as a function of the fixed-point error f, vector tweak or None, the branches
# `decide` must report, in integer mode only (the thresholds need an integer f))
Situation = namedtuple("Situation", "mode state tweak branches integer_only")


def _down(a):
    return math.nextafter(a, 0.0)


def _up(a):
    return math.nextafter(a, INF)


def _tw_primal_small(v, prod):
    v["x_anchor"] = v["x_next"].copy()


def _tw_dual_small(v, prod):
    v["y_anchor"] = v["y_next"].copy()


def _tw_primal_large(v, prod):
    v["x_anchor"][COL0] = 1e12


def _tw_dual_large(v, prod):
    v["y_anchor"][ROW0] = 1e12


def _tw_ratio_high(v, prod):  # one huge reduced cost (x_next is zero there): dFeas / pFeas beyond 1e8
    v["cost"][COL0] = HUGE


def _tw_ratio_low(v, prod):  # one huge right-hand side on an equality row (y_next is zero there)
    v["rhs"][ROW0] = -HUGE


def _tw_rel_p_zero(v, prod):  # every row satisfied exactly: relP == 0
    v["rhs"] = prod["ax"].copy()


SUFF = lambda f: dict(initialFpe=10.0 * f)
NONE = lambda f: dict(initialFpe=f)
SITUATIONS = {
    "first": Situation(1, lambda f: dict(iters=0, hIter=0, nRestarts=0, nChecks=1, initialFpe=0.0), None, ("first", "pid_taken"), False),
    "sufficient": Situation(1, SUFF, None, ("sufficient", "pid_taken", "best_improved"), False),
    "necessary": Situation(1, lambda f: dict(initialFpe=2.0 * f, lastTrialFpe=0.5 * f), None, ("necessary",), False),
    "necessary_not_rising": Situation(1, lambda f: dict(initialFpe=2.0 * f, lastTrialFpe=2.0 * f), None, ("none",), False),
    "artificial": Situation(1, lambda f: dict(initialFpe=f, hIter=120), None, ("artificial",), False),
    "none": Situation(1, NONE, None, ("none",), False),
    # the three thresholds: exactly on them, and one ulp / one iteration to the side that changes the branch
    "sufficient_on": Situation(1, lambda f: dict(initialFpe=5.0 * f), None, ("sufficient",), True),
    "sufficient_past": Situation(1, lambda f: dict(initialFpe=_down(5.0 * f)), None, ("none",), True),
    "sufficient_before": Situation(1, lambda f: dict(initialFpe=_up(5.0 * f)), None, ("sufficient",), True),
    "necessary_on": Situation(1, lambda f: dict(initialFpe=1.25 * f, lastTrialFpe=_down(f)), None, ("necessary",), True),
    "necessary_past": Situation(1, lambda f: dict(initialFpe=_down(1.25 * f), lastTrialFpe=_down(f)), None, ("none",), True),
    "necessary_before": Situation(1, lambda f: dict(initialFpe=_up(1.25 * f), lastTrialFpe=_down(f)), None, ("necessary",), True),
    "last_trial_on": Situation(1, lambda f: dict(initialFpe=2.0 * f, lastTrialFpe=f), None, ("none",), False),
    "last_trial_below": Situation(1, lambda f: dict(initialFpe=2.0 * f, lastTrialFpe=_down(f)), None, ("necessary",), False),
    "artificial_on": Situation(1, lambda f: dict(initialFpe=f, iters=960, hIter=320), None, ("artificial",), False),
    "artificial_below": Situation(1, lambda f: dict(initialFpe=f, iters=960, hIter=319), None, ("none",), False),
    # the PID update of the primal weight and each of its guards
    "pid_primal_small": Situation(1, SUFF, _tw_primal_small, ("sufficient", "pid_refused:primal_small"), False),
    "pid_dual_small": Situation(1, SUFF, _tw_dual_small, ("sufficient", "pid_refused:dual_small"), False),
    "pid_primal_large": Situation(1, SUFF, _tw_primal_large, ("sufficient", "pid_refused:primal_large"), False),
    "pid_dual_large": Situation(1, SUFF, _tw_dual_large, ("sufficient", "pid_refused:dual_large"), False),
    "pid_ratio_high": Situation(1, SUFF, _tw_ratio_high, ("sufficient", "pid_refused:ratio_high"), False),
    "pid_ratio_low": Situation(1, SUFF, _tw_ratio_low, ("sufficient", "pid_refused:ratio_low"), False),
    "pid_rel_p_zero": Situation(1, SUFF, _tw_rel_p_zero, ("sufficient", "pid_refused:ratio_high(relP=0)", "best_kept"), False),
    "best_kept": Situation(1, lambda f: dict(initialFpe=10.0 * f, bestGap=0.0), None, ("sufficient", "pid_taken", "best_kept"), False),
    "pid_off": Situation(1, lambda f: dict(initialFpe=10.0 * f, pid=0), None, ("sufficient", "pid_off"), False),
    # convergence, the iteration limit, the initial fixed-point error of a block behind a restart, a halted loop
    "converged_terminate": Situation(1, lambda f: dict(initialFpe=10.0 * f, tol=1e300), None, ("converged_terminate",), False),
    "converged_ignored": Situation(1, lambda f: dict(initialFpe=10.0 * f, tol=1e300, terminate=0), None, ("converged_ignored", "sufficient"), False),
    "limit_with_restart": Situation(1, lambda f: dict(initialFpe=10.0 * f, iterLimit=440), None, ("sufficient", "limit"), False),
    "limit_no_restart": Situation(1, lambda f: dict(initialFpe=f, iterLimit=440), None, ("none", "limit"), False),
    "limit_fixed_work": Situation(1, lambda f: dict(initialFpe=f, iterLimit=440, terminate=0), None, ("none", "limit"), False),
    "fpe0_set": Situation(2, lambda f: dict(initialFpe=123.0, fpe0Pending=1, runFpe0=1), None, ("fpe0", "none"), False),
    "fpe0_clear": Situation(2, lambda f: dict(initialFpe=10.0 * f), None, ("sufficient",), False),
    "halted": Situation(1, lambda f: dict(initialFpe=10.0 * f, halted=1, run=0, termStatus=1), None, ("halted",), False),
}
VECTOR_SITUATIONS = ("first", "none", "converged_terminate", "limit_with_restart")  # restart due / not, output kept: every size


def situation_state(name, f):
    s = dict(BASE)
    s.update(SITUATIONS[name].state(float(f)))
    return s
