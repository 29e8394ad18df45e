"""Generated problems, planted states and an order-free reference for the 30 sums of a check iteration (4 row and 11 column
statistics, each for the current and the average iterate) and the 20 numbers derived from them: for
tests/test_check_stats_host.py and tests/test_gpu_check_stats.py.  Fixed seeds, nothing read from disk.

The reference is written from the definitions of cuPDLP-C (cupdlp_solver.c: PDHG_Compute_Primal_Feasibility,
PDHG_Compute_Dual_Feasibility, PDHG_Compute_Primal_Infeasibility, PDHG_Compute_Dual_Infeasibility), with numpy on whole
vectors, each step in the order of the reference's vector calls.  Two things differ from that text, both on purpose:
  - the reference divides the two rays by their norms before it squares them; the product (like the reference's own kernel
    build, which passes 1 / norm into the kernel) keeps the sums of the UNSCALED rays and divides afterwards: the sums here are
    those, the division is in `derived`;
  - a QP's terms (q_j x_j and (N x)_j in the reduced cost, 1/2 x'Qx as an eleventh column sum) have no counterpart in
    cuPDLP-C: they follow the objective 1/2 x'Qx + c'x, the diagonal part and the off-diagonal part N added in that order.

Order of the 30 sums (one array, as the device keeps it): rows of the current iterate [0, 4), rows of the average [4, 8),
columns of the current iterate [8, 19), columns of the average [19, 30).
  rows     0 ||rowScale . proj(ax - b)||^2 (proj = min(., 0) on inequality rows)   1 y'b   2 ||y||^2   3 ||rowScale . proj(ax)||^2
  columns  0 c'x   1 s+'l   2 s-'u   3 ||colScale . (r - s+ + s-)||^2   4 ||s+||^2   5 ||s-||^2   6 ||colScale . (aty + s+ - s-)||^2
           7 ||x||^2   8 ||min(x, 0) hasL / colScale||^2   9 ||max(x, 0) hasU / colScale||^2   10 1/2 x'Qx
with r = c - aty (+ q x + N x), s+ = max(r, 0) hasL, s- = -min(r, 0) hasU, l and u with their infinite entries set to zero."""
import math
from collections import namedtuple

import numpy as np

from highs_amd import lp as L

INF = float("inf")
ROW_STATS, COL_STATS = 4, 11
N_STATS = 2 * ROW_STATS + 2 * COL_STATS
ROW_NAMES = ("pres2", "yb", "y2", "ray_ax2")
COL_NAMES = ("cx", "sp_l", "sn_u", "dres2", "sp2", "sn2", "ray_aty2", "x2", "ray_lb2", "ray_ub2", "half_xqx")
NAMES = tuple("%s_%s" % (q, it) for it, group in (("cur", ROW_NAMES), ("avg", ROW_NAMES)) for q in group) + \
    tuple("%s_%s" % (q, it) for it, group in (("cur", COL_NAMES), ("avg", COL_NAMES)) for q in group)
DERIVED_NAMES = ("pObj", "dObj", "gap", "relGap", "pFeas", "dFeas", "pInfObj", "pInfRes", "dInfObj", "dInfRes")
BOUND_KINDS = ("free", "lower", "upper", "boxed", "fixed")

# terms: float64 per-element terms; fsum: their exact sum rounded once; abs_sum: sum |term|; length; exact: (integer data only)
# the value every correct implementation must return, as a Python int — of TWICE the sum for half_xqx, whose terms are
# half-integers
Quantity = namedtuple("Quantity", "terms fsum abs_sum length exact")


# ---- problems -----------------------------------------------------------------------------------------------------------------
def _values(rng, k, values, lo=1):
    """Integer mode: integers with lo <= |v| <= 8; real mode: standard normals."""
    if values == "integer":
        v = rng.integers(lo, 9, size=k).astype(np.float64)
        return v * rng.choice([-1.0, 1.0], size=k)
    assert values == "real", values
    return rng.standard_normal(k)


def bound_vectors(n, values, rng):
    """Column bounds that cycle through free, lower only, upper only, boxed and fixed (column j has kind j % 5)."""
    kind = np.arange(n) % 5
    lo = _values(rng, n, values, lo=0)
    lo = np.where(kind == 3, -np.abs(lo), lo)  # (boxed: lower <= 0, so that the upper bound stays within 8 too)
    width = np.abs(_values(rng, n, values)) + (0.0 if values == "integer" else 0.5)
    lower = np.where((kind == 1) | (kind >= 3), lo, -INF)
    upper = np.where(kind == 2, lo, np.where(kind == 3, lo + width, np.where(kind == 4, lo, INF)))
    return lower, upper


def stats_lp(n, m, values, seed, qp=None, per_col=2.0):
    """n columns, m rows, about per_col (at most 2) entries per column in distinct rows.  Equality rows first (the first half),
    then `>=` rows (one row: an inequality), so that the formulation neither negates a row nor adds a column; column bounds
    cycle through free / lower / upper / boxed / fixed.  values = "integer": every datum is an integer with |v| <= 8.
    qp = "diag": an even-integer (real mode: positive real) diagonal Hessian; qp = "sparse": also one off-diagonal entry in
    every seventh column (|entry| 1, real mode 0.1: diagonally dominant).
    per_col < 2 exists for the one-launch check, which takes at most 64 work blocks of 512 entries per operand."""
    assert 0 < per_col <= 2.0
    rng = np.random.default_rng(seed)
    base = int(per_col)
    count = base + (rng.random(n) < per_col - base)
    if m == 1:
        count = np.minimum(count, 1)
    if count.sum() == 0:
        count[0] = 1
    first = rng.integers(0, m, n)
    second = (first + 1 + rng.integers(0, max(m - 1, 1), n)) % m
    cols = np.concatenate([np.nonzero(count >= 1)[0], np.nonzero(count >= 2)[0]])
    rows = np.concatenate([first[count >= 1], second[count >= 2]])
    order = np.lexsort((rows, cols))
    cols, rows = cols[order], rows[order]
    a_start = np.zeros(n + 1, np.int32)
    a_start[1:] = np.cumsum(np.bincount(cols, minlength=n))
    a_value = _values(rng, len(cols), values)
    n_eq = m // 2
    rhs = _values(rng, m, values, lo=0)
    row_upper = np.where(np.arange(m) < n_eq, rhs, INF)
    lower, upper = bound_vectors(n, values, rng)
    lp = L.HighsLp(n, m, _values(rng, n, values, lo=0), lower, upper, rhs, row_upper, a_start, rows.astype(np.int32), a_value, 1, 0.0,
                   "stats_%d_%d_%s%s%s" % (n, m, values, "_" + qp if qp else "", "_p%g" % per_col if per_col != 2.0 else "")).normalise()
    if qp:
        assert qp in ("diag", "sparse"), qp
        diag = 2.0 * rng.integers(1, 5, n) if values == "integer" else rng.uniform(0.5, 2.0, n)
        if qp == "diag" or n < 8:
            lp.set_diagonal_hessian(diag)
        else:  # lower triangle, column-wise: column j (j % 7 == 0, not the last ones) also holds row j + 3
            has = (np.arange(n) % 7 == 0) & (np.arange(n) + 3 < n)
            q_start = np.concatenate([[0], np.cumsum(1 + has)]).astype(np.int32)
            q_index = np.zeros(q_start[-1], np.int32)
            q_value = np.zeros(q_start[-1])
            q_index[q_start[:-1]] = np.arange(n)
            q_value[q_start[:-1]] = diag
            q_index[q_start[:-1][has] + 1] = np.nonzero(has)[0] + 3
            q_value[q_start[:-1][has] + 1] = (1.0 if values == "integer" else 0.1) * rng.choice([-1.0, 1.0], int(has.sum()))
            lp.hessian = (q_start, q_index, q_value)
    return lp


# (n, m) on the edges of the statistics kernels (256 threads per block, at most 2048 blocks, a final reduction that enters its
# 4-way unrolled loop at 769 partials): the smallest problem | one side below, one above a block | one block each | 257
# blocks | 768 and 769 partials | the last size without the grid-stride loop and the first with it
SIZES = ((1, 1), (255, 257), (256, 256), (65537, 300), (196608, 196609), (524288, 524289))
# The one-launch check exists where the persistent loop has at most 64 workgroups, i.e. at most 64 work blocks of 512 entries
# per operand: at 65537 columns only a thinner matrix qualifies (its 257 virtual blocks then share 64 workgroups)
THIN_PER_COL = 0.25
_lps = {}


def sized_lp(n, m, values, qp=None, thin=False):
    """stats_lp at a size of SIZES, made once."""
    key = (n, m, values, qp, thin)
    if key not in _lps:
        _lps[key] = stats_lp(n, m, values, seed=1000 + n % 997 + m, qp=qp, per_col=THIN_PER_COL if thin else 2.0)
    return _lps[key]


# ---- planted states -----------------------------------------------------------------------------------------------------------
def _magnitude(rng, k, values):
    """Strictly positive: integers in [1, 1000] / |normal| + 0.01."""
    if values == "integer":
        return rng.integers(1, 1001, size=k).astype(np.float64)
    return np.abs(rng.standard_normal(k)) + 0.01


def _free(rng, k, values):
    if values == "integer":
        return rng.integers(-1024, 1025, size=k).astype(np.float64)
    return rng.standard_normal(k)


def planted(data, values, rng):
    """The vectors to plant for the problem data `data` (cost, rhs and, for a QP, qdiag as the device holds them): x, y, ax, aty,
    x_sum, y_sum (and nx for a QP with off-diagonal entries: data["nx"] = True).  ax and aty do not depend on x and y: the
    statistics read the stored vectors.  Every branch of the statistics is hit by construction, in a fixed cycle:
      row i     i % 3 = 0 / 1 / 2: ax - b negative / zero / positive
      column j  (j // 5) % 3 = 0 / 1 / 2: r negative / zero / positive (j % 5 is the bound kind: all 15 pairs occur);
                (j // 15) % 2: x negative / positive
    Integer mode: every entry is an integer in [-1024, 1024]."""
    cost, rhs = data["cost"], data["rhs"]
    n, m = len(cost), len(rhs)
    i, j = np.arange(m), np.arange(n)
    out = {}
    out["ax"] = rhs + np.where(i % 3 == 0, -1.0, np.where(i % 3 == 1, 0.0, 1.0)) * _magnitude(rng, m, values)
    out["y"] = _free(rng, m, values)
    out["x"] = np.where((j // 15) % 2 == 0, -1.0, 1.0) * _magnitude(rng, n, values)
    grad = cost.copy()  # what is added to -aty: c (+ q x + N x), in the order of the statistics
    if data.get("qdiag") is not None:
        grad = grad + data["qdiag"] * out["x"]
    if data.get("nx"):
        out["nx"] = rng.integers(-64, 65, size=n).astype(np.float64) if values == "integer" else rng.standard_normal(n)
        grad = grad + out["nx"]
    # r = -aty + grad: negative / zero / positive (a QP in real mode: the zero class is zero up to rounding only)
    out["aty"] = grad + np.where((j // 5) % 3 == 0, 1.0, np.where((j // 5) % 3 == 1, 0.0, -1.0)) * _magnitude(rng, n, values)
    out["x_sum"] = _free(rng, n, values)
    out["y_sum"] = _free(rng, m, values)
    if values == "integer":
        for k, v in out.items():
            assert np.array_equal(v, np.rint(v)) and np.abs(v).max() <= (1024 if k != "aty" else 2**20), k
    return out


def planted_data(n, m, values, rng):
    """cost, rhs, lower, upper to plant over a problem whose own data do not reach every branch (tests/edge_cases.py: boxed
    columns, real costs): the data of stats_lp."""
    lower, upper = bound_vectors(n, values, rng)
    return dict(cost=_values(rng, n, values, lo=0), rhs=_values(rng, m, values, lo=0), lower=lower, upper=upper)


def plant(S, values, rng, data=False):
    """Plants a state on the DeviceSolver S (data = True: cost, rhs and bounds too); returns what it has set."""
    qoff = _has(S, "nx")
    out = {}
    if data:
        out.update(planted_data(S.n, S.m, values, rng))
        for k in ("cost", "rhs", "lower", "upper"):
            S.set(k, out[k])
    held = dict(cost=S.get("cost", S.n), rhs=S.get("rhs", S.m), qdiag=S.get("qdiag", S.n) if _has(S, "qdiag") else None, nx=qoff)
    vec = planted(held, values, rng)
    for k, v in vec.items():
        S.set(k, v)
    out.update(vec)
    return out


def _has(S, name):
    try:
        S.get(name, S.n)
        return True
    except RuntimeError:
        return False


VECTORS = ("cost", "rhs", "lower", "upper", "x", "y", "ax", "aty", "x_avg", "y_avg", "ax_avg", "aty_avg")


def read_vectors(S, scaled):
    """The inputs of reference_stats as the device holds them (after a check: the averages are the check's own)."""
    rows = ("rhs", "y", "ax", "y_avg", "ax_avg", "row_scale")
    names = VECTORS + (("col_scale", "row_scale") if scaled else ())
    v = {k: S.get(k, S.m if k in rows else S.n) for k in names}
    if _has(S, "qdiag"):
        v["qdiag"] = S.get("qdiag", S.n)
    if _has(S, "nx"):
        v["nx"], v["nx_avg"] = S.get("nx", S.n), S.get("nx_avg", S.n)
    return v


# ---- the reference ------------------------------------------------------------------------------------------------------------
def _quantity(terms, integer, doubled=False):
    terms = np.ascontiguousarray(terms, dtype=np.float64)
    exact = None
    if integer:
        t = terms * (2.0 if doubled else 1.0)
        assert np.array_equal(t, np.rint(t)), "integer data gave a term that is no integer"
        exact = int(t.astype(np.int64).sum())
    return Quantity(terms, math.fsum(terms), math.fsum(np.abs(terms)), len(terms), exact)


def _row_terms(ax, y, b, row_scale, n_eqs, scaled):
    m = len(b)
    ineq = np.arange(m) >= n_eqs
    res = ax + (-1.0) * b  # cupdlp_axpy(-1, rhs, primalResidual)
    res = np.where(ineq, np.minimum(res, 0.0), res)  # cupdlp_projNeg on the inequality rows
    ray = np.where(ineq, np.minimum(ax, 0.0), ax)  # [Ax, min(Gx, 0)]
    if scaled:
        res = res * row_scale
        ray = ray * row_scale
    return [res * res, y * b, y * y, ray * ray]


def _col_terms(x, aty, c, lower, upper, col_scale, qdiag, nx, scaled):
    has_l, has_u = np.where(lower > -INF, 1.0, 0.0), np.where(upper < INF, 1.0, 0.0)
    l_f, u_f = np.where(lower > -INF, lower, 0.0), np.where(upper < INF, upper, 0.0)  # dLowerFiltered, dUpperFiltered
    r = -aty + c  # scaleVector(-1), axpy(1, cost)
    half = np.zeros(len(x))
    if qdiag is not None:
        r = r + qdiag * x
        half = (0.5 * qdiag * x) * x
    if nx is not None:
        r = r + nx
        half = half + (0.5 * nx) * x
    sp = np.maximum(r, 0.0) * has_l  # projPos, edot(hasLower)
    sn = -np.minimum(r, 0.0) * has_u  # projNeg, scaleVector(-1), edot(hasUpper)
    dres = r + (-1.0) * sp
    dres = dres + sn
    ray = (aty + sp) - sn  # dualInfeasConstr: aty, + lb ray, - ub ray
    lb = np.minimum(x, 0.0) * has_l
    ub = np.maximum(x, 0.0) * has_u
    if scaled:
        dres = dres * col_scale
        ray = ray * col_scale
        lb = lb / col_scale  # cupdlp_ediv
        ub = ub / col_scale
    return [x * c, sp * l_f, sn * u_f, dres * dres, sp * sp, sn * sn, ray * ray, x * x, lb * lb, ub * ub, half], sp + 0.0, sn + 0.0


def reference_stats(v, n_eqs, scaled, sense=1.0, offset=0.0, integer=False):
    """The 30 quantities (a list of Quantity in the order of NAMES) and the four slack vectors, from vectors read back from the
    device (read_vectors).  sense and offset enter only the derived numbers (`derived`); they are kept with the result."""
    rs, cs = (v["row_scale"], v["col_scale"]) if scaled else (None, None)
    qd = v.get("qdiag")
    rows_c = _row_terms(v["ax"], v["y"], v["rhs"], rs, n_eqs, scaled)
    rows_a = _row_terms(v["ax_avg"], v["y_avg"], v["rhs"], rs, n_eqs, scaled)
    cols_c, sp_c, sn_c = _col_terms(v["x"], v["aty"], v["cost"], v["lower"], v["upper"], cs, qd, v.get("nx"), scaled)
    cols_a, sp_a, sn_a = _col_terms(v["x_avg"], v["aty_avg"], v["cost"], v["lower"], v["upper"], cs, qd, v.get("nx_avg"), scaled)
    q = [_quantity(t, integer) for t in rows_c + rows_a]
    for group in (cols_c, cols_a):
        q += [_quantity(t, integer, doubled=(k == COL_STATS - 1)) for k, t in enumerate(group)]
    return dict(q=q, slack_pos=sp_c, slack_neg=sn_c, slack_pos_avg=sp_a, slack_neg_avg=sn_a, sense=float(sense), offset=float(offset),
                qp=qd is not None)


def exact_values(ref):
    """Integer data: the 30 sums as float64 (exact: every one is an integer, or a half-integer, below 2^53)."""
    return np.array([q.exact / (2.0 if k in (8 + COL_STATS - 1, N_STATS - 1) else 1.0) for k, q in enumerate(ref["q"])])


def any_order_bound(q):
    """|computed - fsum| for ANY summation order of q.terms: (length + 1) u sum|term| (tests/test_gpu_edges.py has the derivation;
    the terms themselves are computed with the same roundings on both sides — no contraction, IEEE division)."""
    return (q.length + 1) * 2.0**-53 * q.abs_sum * (1 + 1e-6)


def derived(stats30, qp, sense=1.0, offset=0.0):
    """The ten numbers of the current iterate, then the ten of the average (DERIVED_NAMES), from the 30 sums, in float64
    scalar arithmetic: objectives with sense and offset, the two residual norms, the gap, and the two rays' objective and
    residual divided by ||(y, s+, s-)|| and ||x||, each replaced by 1 below 1e-8 (cupdlp_solver.c:229-256, 326-366)."""
    s = [float(t) for t in stats30]
    out = []
    for rs, cs in ((s[0:4], s[8:19]), (s[4:8], s[19:30])):
        p_obj = ((cs[0] + cs[10]) if qp else cs[0]) * sense + offset
        d_obj = (rs[1] + cs[1]) - cs[2]
        if qp:
            d_obj = d_obj - cs[10]
        d_obj = d_obj * sense + offset
        d_scale = math.sqrt(rs[2] + cs[4] + cs[5])
        if d_scale < 1e-8:
            d_scale = 1.0
        p_scale = math.sqrt(cs[7])
        if p_scale < 1e-8:
            p_scale = 1.0
        out += [p_obj, d_obj, p_obj - d_obj, abs(p_obj - d_obj) / (1.0 + abs(p_obj) + abs(d_obj)), math.sqrt(rs[0]), math.sqrt(cs[3]),
                (d_obj - offset) / sense / d_scale, math.sqrt(cs[6]) / d_scale, (p_obj - offset) / sense / p_scale,
                math.sqrt(rs[3] + cs[8] + cs[9]) / p_scale]
    return np.array(out)


# ---- which branches a state reaches -------------------------------------------------------------------------------------------
def branch_classes(v, n_eqs, half="cur"):
    """name -> boolean mask over the rows or columns, for the iterate `half` ("cur" / "avg"): the classes the planted state
    must fill (tests/test_check_stats_host.py)."""
    sfx = "" if half == "cur" else "_avg"
    ax, x, aty = v["ax" + sfx], v["x" + sfx], v["aty" + sfx]
    ineq = np.arange(len(ax)) >= n_eqs
    d = ax + (-1.0) * v["rhs"]
    r = -aty + v["cost"]
    if v.get("qdiag") is not None:
        r = r + v["qdiag"] * x
    if v.get("nx" + sfx) is not None:
        r = r + v["nx" + sfx]
    has_l, has_u = v["lower"] > -INF, v["upper"] < INF
    out = {"row: ax - b < 0": ineq & (d < 0), "row: ax - b = 0": ineq & (d == 0), "row: ax - b > 0": ineq & (d > 0),
           "row: ax < 0": ineq & (ax < 0), "row: ax > 0": ineq & (ax > 0)}
    for bound, mask in (("lower", has_l), ("no lower", ~has_l), ("upper", has_u), ("no upper", ~has_u)):
        out["col: r < 0, " + bound] = mask & (r < 0)
        out["col: r = 0, " + bound] = mask & (r == 0)
        out["col: r > 0, " + bound] = mask & (r > 0)
        out["col: x < 0, " + bound] = mask & (x < 0)
        out["col: x > 0, " + bound] = mask & (x > 0)
    return out
