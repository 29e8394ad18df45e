"""The restart of a check iteration, restated from the text of cuPDLP-C, and planted states that reach exactly one branch of it:
for tests/test_restart_host.py and tests/test_gpu_restart.py.  Problems, planted vectors and the order-free reference of the
check's 30 sums and 20 derived numbers come from tests/check_cases.py.  Fixed seeds, nothing read from disk.

  decide            PDHG_Check_Restart_GPU (cupdlp_restart.c:3-99) with the score of :113-124, and the `LastRestart` numbers a
                    restart records (cupdlp_proj.c:111-132)
  finish            PDHG_Compute_Step_Size_Ratio (cupdlp_step.c:147-176), the sums' reset (cupdlp_proj.c:106-107) and
                    iLastRestartIter (:143); the trial step sizes the product derives from the result (eta, tau, sigma)
  expected_vectors  the contract of PDHG_Restart_Iterate_GPU (cupdlp_proj.c:88-148) on the vectors

Nothing here is taken from pdlp_checkfn.hpp or pdlp_solver.cpp.  `log` / `exp` are the oracle's own restatement
(pdlp_oracle_det_exp_log), everything else is float64 arithmetic in the reference's order of operations."""
import math
from collections import namedtuple

import numpy as np
import scipy.sparse as sp

import check_cases as K
import oraclelib as O
from highs_amd import abi

# iLast = iterates->iLastRestartIter; LR = resobj->d*LastRestart, LC = resobj->d*LastCandidate (primal feasibility, dual
# feasibility, duality gap)
Memory = namedtuple("Memory", "iLast pFeasLR dFeasLR gapLR pFeasLC dFeasLC gapLC")
GAP, PFEAS, DFEAS = (K.DERIVED_NAMES.index(k) for k in ("gap", "pFeas", "dFeas"))
BRANCHES = ("first", "artificial", "sufficient", "necessary", "none")
RESTART_STATE = ("kind", "nRestarts", "iLast", "pFeasLR", "dFeasLR", "gapLR", "pFeasLC", "dFeasLC", "gapLC", "sumPrimalStep", "sumDualStep",
                 "avgW", "avgWx", "haltIter", "nChecks", "lastCheckIter")
STEPS = ("tau", "sigma", "beta", "eta", "primalStep", "dualStep", "sumPrimalStep", "avgW")


# ---- the decision -------------------------------------------------------------------------------------------------------------
def score(beta, p_feas, d_feas, gap):
    """PDHG_Restart_Score_GPU, cupdlp_restart.c:113-124."""
    return math.sqrt(beta * p_feas * p_feas + d_feas * d_feas / beta + gap * gap)


def decide(derived_cur, derived_avg, beta, it, memory, taken=None):
    """(kind, memory'): kind 0 no restart, 1 to the current iterate, 2 to the average.  derived_cur / derived_avg: the ten numbers
    of check_cases.derived for each iterate.  taken: a list that receives the name of the branch (BRANCHES) and the scores."""
    cur = tuple(float(derived_cur[k]) for k in (PFEAS, DFEAS, GAP))
    avg = tuple(float(derived_avg[k]) for k in (PFEAS, DFEAS, GAP))
    beta, it = float(beta), int(it)
    note = taken.append if taken is not None else (lambda _: None)
    if it == memory.iLast:  # :12-22  first call: both records take the current iterate's numbers
        note(("first", {}))
        return 0, Memory(memory.iLast, *cur, *cur)
    mu_cur = score(beta, *cur)  # :24-29
    mu_avg = score(beta, *avg)
    to_current = mu_cur < mu_avg  # :35-41
    mu_cand = mu_cur if to_current else mu_avg
    mus = dict(muCur=mu_cur, muAvg=mu_avg, muCand=mu_cand)
    kind = 1 if to_current else 2
    if (it - memory.iLast) >= 0.36 * it:  # :45  artificial restart
        branch = "artificial"
    else:
        mu_lr = score(beta, memory.pFeasLR, memory.dFeasLR, memory.gapLR)  # :50-53
        mus["muLR"] = mu_lr
        if mu_cand < 0.2 * mu_lr:  # :56  sufficient decay
            branch = "sufficient"
        else:
            mu_lc = score(beta, memory.pFeasLC, memory.dFeasLC, memory.gapLC)  # :61-64
            mus["muLC"] = mu_lc
            if mu_cand < 0.8 * mu_lr and mu_cand > mu_lc:  # :67  necessary decay
                branch = "necessary"
            else:  # :72
                branch = "none"
                kind = 0
    cand = cur if to_current else avg  # :77-85  the candidate is recorded in every branch that has computed one
    lr = (memory.pFeasLR, memory.dFeasLR, memory.gapLR)
    if kind:  # cupdlp_proj.c:111-132: the last-restart numbers are those of the iterate restarted to
        lr = cand
    note((branch, mus))
    return kind, Memory(memory.iLast, *lr, *cand)


# ---- primal weight and step sizes ---------------------------------------------------------------------------------------------
def det_exp_log(x):
    """(exp(x), log(x)) of one float64 as the oracle restates the device's plain-IEEE routines."""
    a, e, lg = np.array([float(x)]), np.zeros(1), np.zeros(1)
    O.oracle().pdlp_oracle_det_exp_log(1, a.ctypes.data_as(abi.c_f64p), e.ctypes.data_as(abi.c_f64p), lg.ctypes.data_as(abi.c_f64p))
    return float(e[0]), float(lg[0])


def log_beta_update(beta, dP2, dD2):
    """dLogBetaUpdate of cupdlp_step.c:168-169, or None where :166 skips the update."""
    dP, dD = math.sqrt(float(dP2)), math.sqrt(float(dD2))
    if not min(dP, dD) > 1e-10:
        return None
    return 0.5 * det_exp_log(dD / dP)[1] + 0.5 * det_exp_log(math.sqrt(beta))[1]


def step_chain(state, beta, adaptive):
    """Everything behind the new beta: cupdlp_step.c:152 (the mean, of the step sizes before), :173-174, then the trial steps
    as the product keeps them: eta = sqrt(primalStep dualStep), and tau, sigma = eta / sqrt(beta), eta sqrt(beta) under the
    adaptive rule, the two step sizes themselves under the fixed one."""
    out = dict(state)
    mean = math.sqrt(state["primalStep"] * state["dualStep"])
    out["beta"] = beta
    out["primalStep"] = mean / math.sqrt(beta)
    out["dualStep"] = out["primalStep"] * beta
    out["eta"] = math.sqrt(out["primalStep"] * out["dualStep"])
    if adaptive:
        out["tau"], out["sigma"] = out["eta"] / math.sqrt(beta), out["eta"] * math.sqrt(beta)
    else:
        out["tau"], out["sigma"] = out["primalStep"], out["dualStep"]
    return out


def finish(state, kind, dP2, dD2, adaptive, it):
    """state: dict with tau, sigma, beta, eta, primalStep, dualStep, sumPrimalStep, sumDualStep, iLast, nRestarts.  The state
    behind the restart of kind `kind` at iteration `it` (kind 0: unchanged)."""
    if not kind:
        return dict(state)
    beta = state["beta"]
    lg = log_beta_update(beta, dP2, dD2)
    if lg is not None:
        e = det_exp_log(lg)[0]
        beta = e * e  # :170
    out = step_chain(state, beta, adaptive)
    out["sumPrimalStep"] = out["sumDualStep"] = 0.0  # cupdlp_proj.c:106-107
    out["iLast"] = int(it)  # :143
    out["nRestarts"] = state["nRestarts"] + 1
    return out


# ---- the vectors --------------------------------------------------------------------------------------------------------------
ITERATE = ("x", "y", "ax", "aty", "nx")


def expected_vectors(v, x_last, y_last, kind, integer=False):
    """v: x, y, ax, aty (nx), x_sum, y_sum as read BEFORE the check and x_avg, y_avg, ax_avg, aty_avg (nx_avg) as the check has
    computed them.  Returns the vectors behind the check and the two squared distances as check_cases.Quantity."""
    out = {}
    names = [k for k in ITERATE if k in v]
    if kind == 0:
        out.update({k: v[k] for k in names})
        out.update(x_sum=v["x_sum"], y_sum=v["y_sum"], x_last=x_last, y_last=y_last, dP2=None, dD2=None)
        return out
    for k in names:
        out[k] = v[k + "_avg"] if kind == 2 else v[k]
    out["x_sum"], out["y_sum"] = np.zeros_like(v["x_sum"]), np.zeros_like(v["y_sum"])
    out["x_last"], out["y_last"] = out["x"], out["y"]
    dx, dy = out["x"] - x_last, out["y"] - y_last
    out["dP2"], out["dD2"] = K._quantity(dx * dx, integer), K._quantity(dy * dy, integer)
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- planted situations -------------------------------------------------------------------------------------------------------
# name -> (iteration, iLast, the iterate planted nearer feasibility, branch, kind, solver options)
#   decay situations: what LR and LC are planted to, as factors (see memory_for)
Situation = namedtuple("Situation", "it iLast near branch kind options")
FIXED = dict(pdlp_features_off=4)  # the adaptive step rule off (pdlp_step_size_strategy is the other solver's option): tau = primalStep
SITUATIONS = {
    "first": Situation(0, 0, "avg", "first", 0, {}),
    "artificial_avg": Situation(7, 0, "avg", "artificial", 2, {}),
    "artificial_cur": Situation(3, 0, "cur", "artificial", 1, {}),
    "sufficient": Situation(40, 30, "avg", "sufficient", 2, {}),
    "not_sufficient_not_necessary": Situation(40, 30, "cur", "none", 0, {}),
    "necessary": Situation(40, 30, "cur", "necessary", 1, {}),
    "too_slow": Situation(40, 30, "avg", "none", 0, {}),
    "artificial_edge_25": Situation(40, 25, "avg", "artificial", 2, {}),  # 15 >= 14.4
    "artificial_edge_26": Situation(40, 26, "avg", "none", 0, {}),  # 14 < 14.4: the decay tests, planted to say no
    "still": Situation(5, 0, "cur", "artificial", 1, {}),
    "fixed_step": Situation(7, 0, "avg", "artificial", 2, FIXED),
    # one entry of x_last off by 0.01 (integer mode: by 1): a distance between the 1e-10 of cupdlp_step.c:166 and 0.1, beta moves
    "nearly_still": Situation(5, 0, "cur", "artificial", 1, {}),
}
MARGIN = 1e-3
JUNK = 7.0  # what LR and LC hold where the branch must not read them (or must overwrite them)


def memory_for(situation, mu_cand):
    """The planted memory.  A record (0, 0, g) has the score |g| exactly, for every beta."""
    s = SITUATIONS[situation]
    if situation == "sufficient":
        lr, lc = mu_cand / (0.2 * (1 - MARGIN)), 2.0 * mu_cand
    elif situation == "not_sufficient_not_necessary":
        lr, lc = mu_cand / (0.2 * (1 + MARGIN)), mu_cand * (1 + MARGIN)
    elif situation == "necessary":
        lr, lc = mu_cand / (0.8 * (1 - MARGIN)), mu_cand * (1 - MARGIN)
    elif situation in ("too_slow", "artificial_edge_25", "artificial_edge_26"):
        lr, lc = mu_cand / (0.8 * (1 + MARGIN)), mu_cand * (1 - MARGIN)
    else:
        return Memory(s.iLast, JUNK, JUNK, JUNK, JUNK, JUNK, JUNK)
    return Memory(s.iLast, 0.0, 0.0, lr, 0.0, 0.0, lc)


def _shrink(a, values):
    """`near`: integer mode the signs (entries in {-1, 0, 1}), real mode a thousandth."""
    return np.sign(a) if values == "integer" else a * 1e-3


def situation_vectors(data, situation, values, rng):
    """The vectors to plant: those of check_cases.planted, one iterate moved near feasibility (real mode: the other one moved
    away as well, by a factor 1000: the problem data are of order one there, in integer mode the planted state is already of
    order 1000), and x_last, y_last."""
    s = SITUATIONS[situation]
    vec = K.planted(data, values, rng)
    cost, rhs = data["cost"], data["rhs"]

    def grad(x, nx):
        g = cost.copy()
        if data.get("qdiag") is not None:
            g = g + data["qdiag"] * x
        if nx is not None:
            g = g + nx
        return g

    def current(f, fdev):
        g0 = grad(vec["x"], vec.get("nx"))
        dev_ax, dev_aty = vec["ax"] - rhs, vec["aty"] - g0
        for k in ("x", "y") + (("nx",) if "nx" in vec else ()):
            vec[k] = f(vec[k])
        vec["ax"] = rhs + fdev(dev_ax)
        vec["aty"] = grad(vec["x"], vec.get("nx")) + fdev(dev_aty)

    def average(f):
        vec["x_sum"], vec["y_sum"] = f(vec["x_sum"]), f(vec["y_sum"])

    # (integer mode: x and y stay within 1024, which keeps every sum of the check exact; the two residuals of the far
    # current iterate grow eightfold, up to 8000: squares below 2^26, sums of 2^20 of them far below 2^53)
    near, far = (lambda a: _shrink(a, values)), (lambda a: a if values == "integer" else a * 1e3)
    far_dev = (lambda a: a * 8.0) if values == "integer" else far
    if s.near == "avg":
        average(near); current(far, far_dev)
    else:
        current(near, near); average(far)
    vec["x_last"] = K._free(rng, len(cost), values)
    vec["y_last"] = K._free(rng, len(rhs), values)
    if situation in ("still", "nearly_still"):
        vec["x_last"] = vec["x"].copy()
    if situation == "nearly_still":
        vec["x_last"][len(cost) // 2] += 1.0 if values == "integer" else 0.01
    if values == "integer":
        for k, a in vec.items():
            assert np.array_equal(a, np.rint(a)) and np.abs(a).max() <= (1024 if k not in ("aty", "ax") else 2**20 if k == "aty" else 2**14), k
    return vec


def matrix_of(P):
    """A of a solver.Prepared (the problem as formulated and scaled on the host; the device holds the same values) by rows."""
    return sp.csr_matrix((P.csr_val, P.csr_idx, P.csr_beg), shape=(P.m, P.n))


def expected_derived(data, vec, A, n_eqs, scales=None, sense=1.0, offset=0.0, integer=False):
    """The 20 derived numbers the check will find on the planted state, on the CPU: the average is x_sum, y_sum themselves
    (plant_restart sets the sums' weights to one), A x_avg and A' y_avg are computed here."""
    v = dict(cost=data["cost"], rhs=data["rhs"], lower=data["lower"], upper=data["upper"])
    v.update({k: vec[k] for k in ITERATE if k in vec})
    v["x_avg"], v["y_avg"] = vec["x_sum"], vec["y_sum"]
    v["ax_avg"], v["aty_avg"] = A @ vec["x_sum"], A.T @ vec["y_sum"]
    assert "nx" not in vec and data.get("qdiag") is None, "LPs only: N x_avg is not restated here"
    if scales is not None:
        v["row_scale"], v["col_scale"] = scales
    ref = K.reference_stats(v, n_eqs, scales is not None, sense, offset, integer=integer)
    assert not integer or all(q.abs_sum < 2.0**53 for q in ref["q"])
    sums = K.exact_values(ref) if integer else np.array([q.fsum for q in ref["q"]])
    return K.derived(sums, False, sense, offset), ref


def plan(data, situation, values, rng, beta, A=None, n_eqs=0, scales=None, sense=1.0, offset=0.0):
    """Everything to plant for `situation`: (vectors, memory, expected derived numbers or None).  The decay situations need the
    candidate's score, so they need A (LPs only); the others plant a memory that must not be read."""
    vec = situation_vectors(data, situation, values, rng)
    needs_mu = situation in ("sufficient", "not_sufficient_not_necessary", "necessary", "too_slow", "artificial_edge_25", "artificial_edge_26")
    der = None
    if A is not None:
        der, _ = expected_derived(data, vec, A, n_eqs, scales, sense, offset, integer=(values == "integer"))
    if not needs_mu:
        return vec, memory_for(situation, 0.0), der
    assert der is not None, "the decay situations need the matrix"
    mu_cur, mu_avg = score(beta, *(der[k] for k in (PFEAS, DFEAS, GAP))), score(beta, *(der[10 + k] for k in (PFEAS, DFEAS, GAP)))
    return vec, memory_for(situation, min(mu_cur, mu_avg)), der


def held_data(S):
    """cost, rhs, bounds (and qdiag, nx) as the DeviceSolver S holds them."""
    return dict(cost=S.get("cost", S.n), rhs=S.get("rhs", S.m), lower=S.get("lower", S.n), upper=S.get("upper", S.n),
                qdiag=S.get("qdiag", S.n) if K._has(S, "qdiag") else None, nx=K._has(S, "nx"))


def plant_restart(S, situation, values, rng, P=None, data=False, sense=1.0, offset=0.0):
    """Brings the DeviceSolver S to the situation's iteration (iterate(k) leaves the check of iteration k pending) and plants
    vectors, the weights of the running sums (one, nothing pending: the average is x_sum, y_sum) and the memory over it.
    P: the problem as solver.Prepared, for the situations that need A.  data = True: cost, rhs and bounds of check_cases.planted_data too.
    Returns (vectors, memory, expected derived numbers or None, beta)."""
    s = SITUATIONS[situation]
    if s.it:
        st = S.iterate(s.it)
        assert st.iters == s.it, (situation, st.iters)
    if data:
        for k, a in K.planted_data(S.n, S.m, values, rng).items():
            S.set(k, a)
    beta = float(S.get("steps", 8)[2])
    held = held_data(S)
    scaled = values != "integer"
    A = scales = None
    if P is not None:
        scales = (S.get("row_scale", S.m), S.get("col_scale", S.n)) if scaled else None
        A = matrix_of(P)
    vec, memory, der = plan(held, situation, values, rng, beta, A, S.n_eqs, scales, sense, offset)
    for k, a in vec.items():
        S.set(k, a)
    S.set("step_sums", [1.0, 1.0, 0.0, 0.0])
    S.set("restart_memory", list(memory))
    return vec, memory, der, beta
