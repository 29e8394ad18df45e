"""Seeded modifications of an LP / QP that pdlp_mi355x_update can express (costs, column bounds, row bounds that keep
every row's kind, offset), for tests/test_update_host.py and tests/test_gpu_update.py.  Each returns the keyword
arguments of DeviceSolver.update / abi.UpdateHandle; `apply` builds the modified problem P' in Python."""
import copy

import numpy as np

INF = 1e20  # |value| >= 1e20 is infinite (CupdlpWrapper.cpp:316-317)
KINDS = ("cost", "col_bounds", "row_bounds", "all")


def row_kind(lo, up):
    """formulate()'s rule: 0 equality, 1 <=, 2 >=, 3 ranged or free."""
    hl, hu = lo > -INF, up < INF
    return np.where(hl & hu & (lo == up), 0, np.where(hl & ~hu, 2, np.where(~hl & hu, 1, 3)))


def new_cost(lp, rng):
    c = np.array(lp.col_cost, dtype=np.float64)
    c = c * (1.0 + 0.3 * rng.standard_normal(c.size))
    k = max(1, c.size // 7)
    c[rng.choice(c.size, k, replace=False)] = rng.standard_normal(k)   # zero costs become nonzero ...
    c[rng.choice(c.size, k, replace=False)] = 0.0                      # ... and the reverse
    return c


def new_col_bounds(lp, rng):
    lo = np.array(lp.col_lower, dtype=np.float64)
    up = np.array(lp.col_upper, dtype=np.float64)
    n = lo.size
    fin_lo, fin_up = lo > -INF, up < INF
    # finite bounds move (and stay ordered)
    shift = 0.25 * rng.random(n)
    lo = np.where(fin_lo, lo - shift, lo)
    up = np.where(fin_up, up + 0.5 * shift, up)
    # x >= 0 columns: some become boxed, some free, some fixed
    plain = np.nonzero((np.asarray(lp.col_lower) == 0.0) & ~fin_up)[0]
    rng.shuffle(plain)
    q = max(1, plain.size // 8) if plain.size else 0
    boxed, free, fixed = plain[:q], plain[q:2 * q], plain[2 * q:3 * q]
    lo[boxed] = 0.0
    up[boxed] = 1.0 + 9.0 * rng.random(boxed.size)
    lo[free] = -np.inf
    up[free] = np.inf
    v = rng.random(fixed.size)
    lo[fixed] = v
    up[fixed] = v
    # an infinite bound becomes finite (and, given as 1e30, a finite one infinite)
    inf_up = np.nonzero(~(up < INF))[0]
    if inf_up.size:
        j = inf_up[rng.integers(inf_up.size)]
        up[j] = (lo[j] if lo[j] > -INF else 0.0) + 5.0
    inf_lo = np.nonzero(~(lo > -INF))[0]
    if inf_lo.size:
        j = inf_lo[rng.integers(inf_lo.size)]
        lo[j] = (up[j] if up[j] < INF else 0.0) - 5.0
    fin = np.nonzero((up < INF) & (lo != up))[0]
    if fin.size:
        up[fin[rng.integers(fin.size)]] = 1e30
    return lo, up


def new_row_bounds(lp, rng):
    """Every row keeps its kind: equalities get a new value, one-sided rows a new bound, ranged rows move both bounds
    (their slack's bounds), a free row may become ranged (both are slack rows)."""
    lo = np.array(lp.row_lower, dtype=np.float64)
    up = np.array(lp.row_upper, dtype=np.float64)
    kind = row_kind(lo, up)
    d = 0.1 + rng.random(lo.size)
    eq, leq, geq = kind == 0, kind == 1, kind == 2
    v = np.where(eq, lo * (1.0 + 0.2 * rng.standard_normal(lo.size)) + 0.01 * d, 0.0)
    lo = np.where(eq, v, lo)
    up = np.where(eq, v, up)
    up = np.where(leq, up + d, up)
    lo = np.where(geq, lo - d, lo)
    ranged = (kind == 3) & (lo > -INF) & (up < INF)
    lo = np.where(ranged, lo - 0.5 * d, lo)
    up = np.where(ranged, up + 0.25 * d, up)
    free = np.nonzero((kind == 3) & ~(lo > -INF) & ~(up < INF))[0]
    if free.size:
        i = free[rng.integers(free.size)]
        lo[i], up[i] = -3.0, 4.0
    assert np.array_equal(row_kind(lo, up), kind)
    return lo, up


def modification(lp, what, seed):
    rng = np.random.default_rng(seed)
    u = {}
    if what in ("cost", "all"):
        u["col_cost"] = new_cost(lp, rng)
    if what in ("col_bounds", "all"):
        u["col_lower"], u["col_upper"] = new_col_bounds(lp, rng)
    if what in ("row_bounds", "all"):
        u["row_lower"], u["row_upper"] = new_row_bounds(lp, rng)
    if what == "all":
        u["offset"] = float(lp.offset) + 1.5
    return u


def apply(lp, u):
    """The modified problem P' (a copy; the matrix arrays are shared)."""
    out = copy.copy(lp)
    for k, v in u.items():
        if k == "offset":
            out.offset = float(v)
        elif k != "start":
            setattr(out, k, np.array(v, dtype=np.float64))
    return out
