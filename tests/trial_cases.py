"""Problems, planted states and an elementwise restatement of ONE trial of solver="pdlp" — the primal step, the dual step, the
three or four grid-wide sums, the accept / reject decision with everything it leaves in the device's state record, and the
deferred updates of the running sums — for tests/test_trial_host.py and tests/test_gpu_trial.py.  Fixed seeds, nothing read from
disk.

The restatement is numpy float64 on whole vectors, every step in the order of cuPDLP-C's vector calls (cupdlp_step.c:16-69
PDHG_primalGradientStep / PDHG_dualGradientStep, cupdlp_linalg.c:772-801 the movement and the interaction, cupdlp_step.c:237-306
the adaptive rule, :422-442 PDHG_Update_Average) and of the record decideCore (pdlp_devfn.hpp) keeps.  It knows nothing of work
blocks, lanes, reduction trees or the oracle.  What has no counterpart in cuPDLP-C — a QP's prox division by 1 + tau q_j, the
explicit term -tau (N x)_j, dx . N dx and its half in the step limit — follows the objective 1/2 x'Qx + c'x, Q = diag(q) + N.

The sums are compared without an order:
  integer data, no scaling, tau and sigma powers of two: every x+, y+, A x+, A'y+, N x+ and every term is a multiple of one power
      of two, every sum of them below 2^53 such units — exact in ANY order, so `==` (exact_sum asserts the premise);
  real data: |device - fsum(terms)| <= (k + 1) 2^-53 sum|term| (1 + 1e-6) for k terms, the any-order bound of
      tests/test_gpu_edges.py, the terms formed elementwise from the device's own vectors.

trial_state (Solver::getVector / setVector): the 27 scalars of DevState in the order of STATE."""
import math

import numpy as np

import check_cases as K
from highs_amd import lp as L

INF = float("inf")
U = 2.0**-53
STATE = ("eta", "beta", "tau", "sigma", "primalStep", "dualStep", "sumPrimalStep", "sumDualStep", "avgW", "avgWx", "dX2", "dY2", "inter",
         "movement", "limit", "qint", "nIter", "nTrials", "cur", "halted", "haltIter", "adaptive", "lastAccepted", "powBase", "powCount",
         "commError", "pending")
INT_FIELDS = STATE[16:]
INT_MAX = 2**31 - 1
POW_WINDOW, POW_MARGIN = 16384, 4096  # Solver::refreshPowTable


def state_dict(arr):
    assert len(arr) == len(STATE)
    return {k: (int(v) if k in INT_FIELDS else float(v)) for k, v in zip(STATE, arr)}


def state_array(state):
    return np.array([float(state[k]) for k in STATE])


# ---- problems -----------------------------------------------------------------------------------------------------------------
def circulant_lp(n, offsets, values, seed, qp=None, q_offset=5):
    """n columns, n rows; column j holds the rows (j + d) % n, d in offsets: every row and every column has len(offsets) entries,
    so an operand of len(offsets) * n entries has EXACTLY ceil(len(offsets) * n / chunk) work blocks (the planner closes a block
    at `chunk` entries: tests/test_trial_host.py asks it).  Rows: the first half equalities, then `>=`; column bounds cycle as in
    check_cases.  qp = "sparse": diagonal plus the symmetric off-diagonal entries (j, (j + q_offset) % n) — N has two entries
    in every row."""
    rng = np.random.default_rng(seed)
    k = len(offsets)
    assert len(set(d % n for d in offsets)) == k
    rows = (np.arange(n)[:, None] + np.asarray(offsets)[None, :]) % n
    rows.sort(axis=1)
    a_start = (np.arange(n + 1) * k).astype(np.int32)
    a_value = K._values(rng, n * k, values)
    rhs = K._values(rng, n, values, lo=0)
    row_upper = np.where(np.arange(n) < n // 2, rhs, INF)
    lower, upper = K.bound_vectors(n, values, rng)
    lp = L.HighsLp(n, n, K._values(rng, n, values, lo=0), lower, upper, rhs, row_upper, a_start, rows.reshape(-1).astype(np.int32), a_value, 1, 0.0,
                   "circulant_%d_%d_%s%s" % (n, k, values, "_" + qp if qp else "")).normalise()
    if qp:
        assert qp == "sparse" and 0 < q_offset < n - q_offset
        diag = 2.0 * rng.integers(1, 5, n) if values == "integer" else rng.uniform(0.5, 2.0, n)
        j = np.arange(n)
        other = (j + q_offset) % n
        col, row = np.minimum(j, other), np.maximum(j, other)  # lower triangle: row > column
        off = (1.0 if values == "integer" else 0.1) * rng.choice([-1.0, 1.0], n)
        col = np.concatenate([j, col]); row = np.concatenate([j, row]); val = np.concatenate([diag, off])
        order = np.lexsort((row, col))
        q_start = np.zeros(n + 1, np.int32)
        q_start[1:] = np.cumsum(np.bincount(col, minlength=n))
        lp.hessian = (q_start, row[order].astype(np.int32), val[order])
    return lp


# case -> (maker(values, qp), the QP variants it has).  Work blocks per operand (asserted on the planner by the host test):
#   1x1, 255x257, 256x256   one block of 512 entries each
#   65537x300               A 300 blocks (one row each), A' 257
#   blocks256 / blocks257   A and A' (and N of the QP) exactly 256 / 257 blocks of 512 entries: the last count with one partial
#                           per lane in trialSumsT and the first with two
#   wide257 ... wide1025    operands of >= 2^18 entries, blocks of 2048: 257 (two partials in lane 0), 768 / 769 (`four`'s and
#                           laneSum's full round starts where tid + 768 < count), 1024 / 1025 (the last count of WIDE, the first
#                           of a second round)
CASES = {
    "1x1": (lambda v, qp: K.sized_lp(1, 1, v, qp), ("diag",)),
    "255x257": (lambda v, qp: K.sized_lp(255, 257, v, qp), ("diag", "sparse")),
    "256x256": (lambda v, qp: K.sized_lp(256, 256, v, qp), ("diag", "sparse")),
    "65537x300": (lambda v, qp: K.sized_lp(65537, 300, v, qp), ("diag", "sparse")),
    "blocks256": (lambda v, qp: circulant_lp(256 * 256, (0, 37), v, 256, qp), ("sparse",)),
    "blocks257": (lambda v, qp: circulant_lp(256 * 257, (0, 37), v, 257, qp), ("sparse",)),
}
WIDE_OFFSETS = tuple(range(0, 16 * 41, 41))  # sixteen entries per row and column: 128 columns per block of 2048
for _b in (257, 768, 769, 1024, 1025):
    CASES["wide%d" % _b] = ((lambda b: lambda v, qp: circulant_lp(128 * b, WIDE_OFFSETS, v, b, qp))(_b), ())
BLOCKS = {"1x1": (1, 1, 512), "255x257": (1, 1, 512), "256x256": (1, 1, 512), "65537x300": (300, 257, 512), "blocks256": (256, 256, 512),
          "blocks257": (257, 257, 512), **{"wide%d" % b: (b, b, 2048) for b in (257, 768, 769, 1024, 1025)}}
_lps = {}


def lp_of(case, values, qp=None):
    key = (case, values, qp)
    if key not in _lps:
        assert qp is None or qp in CASES[case][1], key
        _lps[key] = CASES[case][0](values, qp)
    return _lps[key]


def options(values):
    return dict(pdlp_features_off=1) if values == "integer" else {}


def matrices(lp):
    """(rows, cols, vals) of A as the LP gives it (the formulation of these problems neither permutes nor negates: asserted by the
    host test), and of the off-diagonal part N of a QP's Hessian, both triangles, or None."""
    cols = np.repeat(np.arange(lp.num_col), np.diff(lp.a_start))
    A = (np.asarray(lp.a_index, dtype=np.int64), cols, np.asarray(lp.a_value, dtype=np.float64))
    N = None
    h = getattr(lp, "hessian", None)
    if h is not None:
        q_start, q_index, q_value = h
        qc = np.repeat(np.arange(lp.num_col), np.diff(q_start))
        qr = np.asarray(q_index, dtype=np.int64)
        offd = qr != qc
        if offd.any():
            N = (np.concatenate([qr[offd], qc[offd]]), np.concatenate([qc[offd], qr[offd]]), np.concatenate([q_value[offd], q_value[offd]]))
    return A, N


def matvec(M, v, n_out, transpose=False):
    """M v (or M' v) by one product per entry and a sum per row.  Only used where every product and every partial sum is exact
    (integer data), so its summation order does not matter."""
    r, c, a = M
    if transpose:
        r, c = c, r
    return np.bincount(r, weights=a * v[c], minlength=n_out).astype(np.float64)


# ---- the restatement: vectors -------------------------------------------------------------------------------------------------
def primal_step(x, aty, cost, lower, upper, tau, qdiag=None, nx=None):
    """cupdlp_step.c:16-40 on the CPU branch: copy, axpy(-tau, c), axpy(tau, A'y), (QP: axpy(-tau, N x), the prox division), projub,
    projlb."""
    t = x.copy()
    t = t + (-tau) * cost
    t = t + tau * aty
    if nx is not None:
        t = t + (-tau) * nx
    if qdiag is not None:
        t = t / (1.0 + tau * qdiag)
    t = np.where(t < upper, t, upper)
    t = np.where(t > lower, t, lower)
    return t


def dual_step(y, ax, ax_next, rhs, sigma, n_eqs):
    """cupdlp_step.c:43-69: copy, axpy(sigma, b), axpy(-2 sigma, A x+), axpy(sigma, A x), projPos on the inequality rows."""
    t = y.copy()
    t = t + sigma * rhs
    t = t + (-2.0 * sigma) * ax_next
    t = t + sigma * ax
    ineq = np.arange(len(y)) >= n_eqs
    return np.where(ineq, np.where(t > 0.0, t, 0.0), t)


def sum_terms(v, nxt):
    """The terms of the sums from the iterate v and the trial point nxt (dicts of vectors): (dx)^2, (dy)^2, dx . d(A'y) and, with
    nx, dx . d(N x): cupdlp_linalg.c:772-801, the differences taken current minus next."""
    dx = v["x"] - nxt["x"]
    dy = v["y"] - nxt["y"]
    out = dict(dX2=dx * dx, dY2=dy * dy, inter=dx * (v["aty"] - nxt["aty"]))
    if v.get("nx") is not None:
        out["qint"] = dx * (v["nx"] - nxt["nx"])
    return out


def exact_sum(terms):
    """Integer data: the sum every order must give.  The terms are multiples of one power of two (the weight of the lowest set
    bit of any of them) and the sum of their magnitudes stays below 2^53 such units, so every partial sum of every order is
    exact; fsum returns that sum."""
    terms = np.asarray(terms, dtype=np.float64)
    nz = terms[terms != 0.0]
    if len(nz) == 0:
        return 0.0
    mant, exp = np.frexp(np.abs(nz))
    bits = (mant * 2.0**53).astype(np.int64)  # exact: a mantissa has 53 bits
    low = np.frexp((bits & -bits).astype(np.float64))[1] - 1  # position of the lowest set bit
    unit = 2.0 ** int((exp - 53 + low).min())
    scaled = nz / unit
    assert np.array_equal(scaled, np.rint(scaled)) and math.fsum(np.abs(scaled)) < 2.0**53, "the terms leave the exact grid"
    return math.fsum(nz)


def any_order_bound(terms):
    terms = np.asarray(terms, dtype=np.float64)
    return math.fsum(terms), (len(terms) + 1) * U * math.fsum(np.abs(terms)) * (1 + 1e-6)


def restate_trial(lp, v, tau, sigma, n_eqs):
    """Integer data: the whole trial point from the iterate v (x, y, ax, aty, nx) and the problem data in v (cost, rhs, lower, upper,
    qdiag): x+, A x+, y+, A'y+, N x+ and the exact sums."""
    A, N = matrices(lp)
    n, m = len(v["x"]), len(v["y"])
    nxt = {}
    nxt["x"] = primal_step(v["x"], v["aty"], v["cost"], v["lower"], v["upper"], tau, v.get("qdiag"), v.get("nx"))
    nxt["ax"] = matvec(A, nxt["x"], m)
    nxt["y"] = dual_step(v["y"], v["ax"], nxt["ax"], v["rhs"], sigma, n_eqs)
    nxt["aty"] = matvec(A, nxt["y"], n, transpose=True)
    if v.get("nx") is not None:
        nxt["nx"] = matvec(N, nxt["x"], n)
    sums = {k: exact_sum(t) for k, t in sum_terms(v, nxt).items()}
    sums.setdefault("qint", 0.0)
    return nxt, sums


# ---- the restatement: the decision ----------------------------------------------------------------------------------------------
def decide(state, dX2, dY2, inter, qint=0.0, branch=None):
    """cupdlp_step.c:259-306 with the record of decideCore: the full state a trial with these sums leaves.  The powers are
    math.pow's (glibc's, as the host tabulates them).  branch (a dict) receives which way each choice went."""
    s = dict(state)
    sb = math.sqrt(s["beta"])
    movement = dX2 * 0.5 * sb + dY2 / (2.0 * sb)
    s["nTrials"] += 1
    accept, eta_new, limit = True, s["eta"], INF
    taken = {}
    if s["adaptive"]:
        den = abs(inter) + 0.5 * abs(qint)
        limit = movement / den if den != 0.0 else INF
        accept = s["eta"] <= limit
        k1 = float(s["nTrials"]) + 1.0
        first = (1.0 - math.pow(k1, -0.3)) * limit
        second = (1.0 + math.pow(k1, -0.6)) * s["eta"]
        eta_new = min(first, second)
        taken.update(den_zero=den == 0.0, first_wins=first < second, second_wins=second < first, first=first, second=second)
    s.update(dX2=dX2, dY2=dY2, inter=inter, movement=movement, limit=limit, qint=qint, lastAccepted=int(accept), pending=0)
    if accept:
        if s["adaptive"]:
            s["primalStep"] = eta_new / math.sqrt(s["beta"])
            s["dualStep"] = eta_new * math.sqrt(s["beta"])
        w = math.sqrt(s["primalStep"] * s["dualStep"])  # the NEXT step sizes (cupdlp_step.c:433)
        s["sumPrimalStep"] += w
        s["sumDualStep"] += w
        s["avgW"] = s["avgWx"] = w
        s["cur"] ^= 1
        s["nIter"] += 1
        s["eta"] = w
        if s["nIter"] >= s["haltIter"]:
            s["halted"] = 1
    else:
        s["eta"] = eta_new
        s["avgW"] = s["avgWx"] = 0.0
    if s["adaptive"]:
        s["tau"] = s["eta"] / math.sqrt(s["beta"])
        s["sigma"] = s["eta"] * math.sqrt(s["beta"])
    taken.update(accepted=accept, halted=bool(s["halted"]))
    if branch is not None:
        branch.update(taken)
    return s


def pow_table_after_push(n_trials, base, count):
    """Solver::refreshPowTable: (powBase, powCount) behind a push of the state with this trial counter."""
    if count and n_trials >= base and n_trials + POW_MARGIN < base + count:
        return base, count
    return n_trials, POW_WINDOW


def covered(state):
    """The trial that raises nTrials by one finds its powers in the table."""
    ti = state["nTrials"] + 1 - state["powBase"]
    return 0 <= ti < state["powCount"]


# ---- the restatement: the running sums ------------------------------------------------------------------------------------------
def flushed(x_sum, x_cur, w):
    """The running sum with a pending weight applied: PDHG_Update_Average's axpy (cupdlp_step.c:437-438), one product and one sum
    per element.  Whichever launch applies it — the next primal step, the next dual step, the fused tail, the flush in front of
    a check — this is the sum the reference holds at that point."""
    return x_sum + w * x_cur if w != 0.0 else x_sum.copy()


def average(total, weight):
    """PDHG_Compute_Average_Iterate, cupdlp_step.c:377-420: scaled by 1 / weight (1 where nothing has been summed)."""
    return total * (1.0 / weight if weight > 0.0 else 1.0)


# ---- planted iterates -----------------------------------------------------------------------------------------------------------
def planted_iterate(lp, data, values, rng, n_eqs, kind="natural"):
    """x (inside its bounds), y (>= 0 on the inequality rows), ax, aty (and nx) to plant.  ax, aty and nx are free inputs of a
    trial: it reads the stored vectors.  Integer mode: integers of magnitude <= 64.
      natural         independent random vectors
      consistent_aty  aty = A'y (integer mode: exact), so that a dual step that moves nothing leaves d(A'y) = 0
      positive_inter  aty = A'y, ax = -8 A (c - aty): dx ~ tau (c - aty), d(A'y) ~ 8 sigma A'A (c - aty), the interaction > 0
      negative_inter  aty = c - g with a large g and (the caller's) small sigma: dx ~ tau g and d(A'y) ~ -g, the interaction < 0
      positive_qint / negative_qint   (nx) nx = 8 x / -8 x: the prox division by 1 + tau q_j >= 2 makes dx ~ x (1 - 1 / (1 + tau q_j)),
                      and d(N x) ~ nx, so dx . N dx takes the sign of nx . x"""
    n, m = len(data["cost"]), len(data["rhs"])

    def free(k, top=64):
        return rng.integers(-top, top + 1, size=k).astype(np.float64) if values == "integer" else rng.standard_normal(k) * (top / 64.0)

    out = {}
    out["x"] = np.clip(free(n), data["lower"], data["upper"])
    y = free(m)
    y[n_eqs:] = np.abs(y[n_eqs:])
    out["y"] = y
    out["ax"] = free(m)
    out["aty"] = free(n)
    if data.get("nx"):
        out["nx"] = free(n)
    if kind == "negative_inter":
        g = free(n) + np.where(rng.random(n) < 0.5, -200.0, 200.0)
        out["aty"] = data["cost"] - g
        if "nx" in out:
            out["nx"] = np.zeros(n)
    elif kind in ("positive_qint", "negative_qint"):
        out["nx"] = (8.0 if kind == "positive_qint" else -8.0) * out["x"]
    elif kind in ("consistent_aty", "positive_inter"):
        assert values == "integer"
        A = matrices(lp)[0]
        out["aty"] = matvec(A, out["y"], n, transpose=True)
        if kind == "positive_inter":
            out["ax"] = -8.0 * matvec(A, data["cost"] - out["aty"], m)
    else:
        assert kind == "natural", kind
    out["x_sum"] = free(n)
    out["y_sum"] = free(m)
    return out


def dyadic_qdiag(n, rng, tau=2.0**-4):
    """A diagonal Hessian to plant over the problem's own in integer mode: 1 + tau q_j in {2, 4, 8}, so that the prox division of
    the primal step stays on the grid (q_j = 16, 48 or 112 at tau = 2^-4; tau = 0 divides by one whatever q is)."""
    return (2.0 ** rng.integers(1, 4, n) - 1.0) / tau


# ---- situations -------------------------------------------------------------------------------------------------------------------
# name -> (iterate kind, tau, sigma, beta, what to plant once the trial's sums are known, the branch it must reach).
# eta is planted on its own: the decision reads s.eta and never recomputes it from tau and sigma, so a threshold can be hit
# without solving eta = limit(tau(eta), sigma(eta)).
BASE = dict(beta=4.0, primalStep=0.25, dualStep=0.5, sumPrimalStep=3.0, sumDualStep=5.0, avgW=0.0, avgWx=0.0, dX2=-1.0, dY2=-1.0, inter=-1.0,
            movement=-1.0, limit=-1.0, qint=-1.0, nIter=3, nTrials=7, cur=0, halted=0, haltIter=INT_MAX, adaptive=1, lastAccepted=-1)


def limit_of(sums, beta, with_q=True):
    sb = math.sqrt(beta)
    movement = sums["dX2"] * 0.5 * sb + sums["dY2"] / (2.0 * sb)
    den = abs(sums["inter"]) + (0.5 * abs(sums["qint"]) if with_q else 0.0)
    return movement / den if den != 0.0 else INF


SITUATIONS = {
    # name: (kind, tau, sigma, state overrides as a function of the limit, expected accepted)
    "on_limit": ("positive_inter", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim), True),
    "ulp_below": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=math.nextafter(lim, 0.0)), True),
    "ulp_above": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=math.nextafter(lim, INF)), False),
    "second_wins": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim / 1024.0), True),
    "far_above": ("positive_inter", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim * 1024.0), False),
    "still": ("natural", 0.0, 0.0, lambda lim: dict(eta=0.5), True),
    "moving_no_interaction": ("consistent_aty", 2.0**-4, 0.0, lambda lim: dict(eta=0.5), True),
    "negative_inter": ("negative_inter", 2.0**-4, 2.0**-12, lambda lim: dict(eta=lim), True),
    "negative_inter_rejected": ("negative_inter", 2.0**-4, 2.0**-12, lambda lim: dict(eta=math.nextafter(lim, INF)), False),
    "fixed_step": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim * 1024.0, adaptive=0), True),
    "halts": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim, nIter=39, haltIter=40), True),
    "one_short_of_halt": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim, nIter=38, haltIter=40), True),
    "rejected_at_halt": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim * 2.0, nIter=39, haltIter=40), False),
    "trials_0": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim, nTrials=0), True),
    "trials_1": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim * 2.0, nTrials=1), False),
    "trials_12287": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim, nTrials=12287), True),
    "trials_12288": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim * 2.0, nTrials=12288), False),
    "trials_1e6": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim, nTrials=10**6), True),
    "pending_weights": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim, avgW=0.75, avgWx=0.75), True),
    "pending_weights_rejected": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim * 2.0, avgW=0.75, avgWx=0.75), False),
}
# a QP with off-diagonal Hessian entries: dx . N dx alone turns an accept into a reject; its sign
QP_SITUATIONS = {
    "qint_rejects": ("natural", 2.0**-4, 2.0**-5, lambda lim: dict(eta=math.nextafter(lim, INF)), False),
    "qint_on_limit": ("positive_qint", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim), True),
    "negative_qint": ("negative_qint", 2.0**-4, 2.0**-5, lambda lim: dict(eta=lim), True),
    "negative_qint_rejected": ("negative_qint", 2.0**-4, 2.0**-5, lambda lim: dict(eta=math.nextafter(lim, INF)), False),
}
# that cannot be den == 0 with off-diagonal entries (dx . N dx != 0 wherever dx != 0 on these problems)
LP_ONLY = ("moving_no_interaction",)
ALL_SITUATIONS = dict(SITUATIONS, **QP_SITUATIONS)


def situation_state(name, sums):
    """The state to plant for the situation, given the exact sums its (tau, sigma) produce on the planted iterate."""
    kind, tau, sigma, make, accepted = ALL_SITUATIONS[name]
    s = dict(BASE, tau=tau, sigma=sigma)
    s.update(make(limit_of(sums, s["beta"])))
    s.update(powBase=0, powCount=0, commError=0, pending=0)
    return s


def claims(name, state, sums):
    """What the situation claims about itself, as booleans: all must hold (tests/test_trial_host.py, and again on the device's
    sums in tests/test_gpu_trial.py)."""
    taken = {}
    after = decide(state, sums["dX2"], sums["dY2"], sums["inter"], sums["qint"], taken)
    lim = after["limit"]
    out = {"accepted as claimed": taken["accepted"] == ALL_SITUATIONS[name][4]}
    if name in ("on_limit", "qint_on_limit", "negative_inter", "negative_qint"):
        out["eta == limit"] = state["eta"] == lim and math.isfinite(lim)
    if name == "on_limit":
        out["first wins"] = taken["first_wins"]
    if name == "ulp_below":
        out["one ulp below"] = math.nextafter(state["eta"], INF) == lim
    if name in ("ulp_above", "qint_rejects", "negative_inter_rejected", "negative_qint_rejected"):
        out["one ulp above"] = math.nextafter(state["eta"], 0.0) == lim
    if name == "second_wins":
        out["second wins"] = taken["second_wins"]
    if name == "still":
        out["nothing moves"] = sums["dX2"] == 0.0 and sums["dY2"] == 0.0 and taken["den_zero"] and lim == INF
    if name == "moving_no_interaction":
        out["moves without interaction"] = sums["inter"] == 0.0 and sums["qint"] == 0.0 and after["movement"] > 0.0 and lim == INF
    if name.startswith("negative_inter"):
        out["inter < 0"] = sums["inter"] < 0.0
    if name == "on_limit" or name == "far_above":
        out["inter > 0"] = sums["inter"] > 0.0
    if name == "qint_rejects":
        out["accepted without qint"] = sums["qint"] != 0.0 and state["eta"] <= limit_of(sums, state["beta"], with_q=False)
    if name == "qint_on_limit":
        out["qint > 0"] = sums["qint"] > 0.0
    if name.startswith("negative_qint"):
        out["qint < 0"] = sums["qint"] < 0.0
    if name == "fixed_step":
        out["would be rejected"] = state["eta"] > limit_of(sums, state["beta"]) and after["limit"] == INF and after["tau"] == state["tau"]
    if name == "halts":
        out["halts"] = after["halted"] == 1 and after["nIter"] == state["haltIter"]
    if name == "one_short_of_halt":
        out["does not halt"] = after["halted"] == 0 and after["nIter"] + 1 == state["haltIter"]
    if name == "rejected_at_halt":
        out["does not halt"] = after["halted"] == 0 and after["nIter"] + 1 == state["haltIter"]
    return out, after
