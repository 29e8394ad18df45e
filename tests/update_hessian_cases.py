"""Seeded changes of the Hessian VALUES of a QP on its created sparsity pattern, as pdlp_mi355x_update_values takes them,
for tests/test_update_hessian_host.py and tests/test_gpu_update_hessian.py.  `new_values` returns q_value in the positions
of lp.hessian's values: positions that a regenerated Q does not fill are 0.0, and nothing that would need a new slot is
generated.  `modification` returns the keyword arguments of DeviceSolver.update_values; `apply` builds the modified
problem P' in Python (a helper, not a conftest)."""
import copy

import numpy as np

import update_matrix_cases as MC

KINDS = ("scale0.3", "scale7", "regen", "diag_only", "zero_off", "all")


def _slots(lp):
    st, idx, _ = lp.hessian
    st = np.asarray(st, dtype=np.int64)
    rows = np.asarray(idx, dtype=np.int64)
    cols = np.repeat(np.arange(len(st) - 1, dtype=np.int64), np.diff(st))
    return rows, cols


def _fill(lp, Q):
    """The dense symmetric Q into the created pattern (repeated pairs: the first slot takes the value, the rest 0.0)."""
    rows, cols = _slots(lp)
    q = np.zeros(rows.size)
    seen = set()
    for p, (i, j) in enumerate(zip(rows.tolist(), cols.tolist())):
        if (i, j) not in seen:
            q[p] = Q[i, j]
            seen.add((i, j))
    need = np.tril(Q != 0.0)
    need[rows, cols] = False
    assert not need.any(), "the regenerated Hessian would need a new slot"
    return q


def _regen_sparse(lp, seed, gen_seed):
    """lpgen.random_sparse_qp(gen_seed) again: G's nonzeros redrawn on G's pattern, Q' = G''G' + diag(d'), still PSD."""
    nc = lp.num_col
    rng0 = np.random.default_rng(2000 + gen_seed)  # the generator's stream: G's and d's pattern
    k = max(2, nc // 2)
    dens = min(0.5, 3.0 / nc)
    g_pattern = (rng0.standard_normal((k, nc)) * (rng0.random((k, nc)) < dens)) != 0.0
    d_pattern = ~(rng0.random(nc) < 0.35)
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((k, nc)) * g_pattern
    d = np.where(d_pattern, rng.uniform(0.1, 2.0, nc), 0.0)
    return _fill(lp, lp.sense * (G.T @ G + np.diag(d)))


def _regen_dominant(lp, seed):
    """Any pattern: the off-diagonal values redrawn in (-0.5, 0.5), every diagonal slot of a column an equal share of the
    absolute sums of its row and column plus U(0, 1) — diagonally dominant, so PSD (times the sense)."""
    rng = np.random.default_rng(seed)
    rows, cols = _slots(lp)
    n = lp.num_col
    q = rng.uniform(-0.5, 0.5, rows.size)
    diag = rows == cols
    q[diag] = 0.0
    dom = np.zeros(n)
    np.add.at(dom, rows[~diag], np.abs(q[~diag]))
    np.add.at(dom, cols[~diag], np.abs(q[~diag]))
    share = np.maximum(np.bincount(cols[diag], minlength=n), 1)
    q[diag] = ((dom + rng.uniform(0.0, 1.0, n)) / share)[cols[diag]]
    return lp.sense * q


def new_values(lp, what, seed, sparse_seed=None):
    """sparse_seed: the seed lp was made with by lpgen.random_sparse_qp (then `regen` redraws its G), else None."""
    rows, cols = _slots(lp)
    q0 = np.array(lp.hessian[2], dtype=np.float64)
    if what.startswith("scale"):
        return float(what[5:]) * q0
    if what == "regen":
        return _regen_sparse(lp, seed, sparse_seed) if sparse_seed is not None else _regen_dominant(lp, seed)
    if what == "diag_only":  # every diagonal slot grows (PSD stays), the off-diagonal values are those of create
        rng = np.random.default_rng(seed)
        q = q0.copy()
        diag = rows == cols
        q[diag] = q0[diag] * rng.uniform(1.0, 4.0, int(diag.sum()))
        return q
    if what == "zero_off":
        return np.where(rows == cols, q0, 0.0)
    raise ValueError(what)


def modification(lp, what, seed, sparse_seed=None):
    if what == "all":
        u = dict(q_value=new_values(lp, "regen", seed, sparse_seed))
        u.update(MC.modification(lp, "all", seed + 1))
        return u
    return dict(q_value=new_values(lp, what, seed, sparse_seed))


def doubly_wrong(lp):
    """Three updates that are each wrong in two ways, name -> (keyword arguments of update_values, words of the refusal that
    must win): a changed kind of row 0, an all-zero a_value and a negative Hessian diagonal are refused in this order."""
    lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
    if MC.UC.row_kind(lo[:1], up[:1])[0] == 0:
        up[0] = np.inf  # equality -> >=
    else:
        lo[0] = up[0] = 1.0  # anything else -> equality
    rows, cols = _slots(lp)
    q_bad = np.array(lp.hessian[2], dtype=np.float64)
    q_bad[np.nonzero(rows == cols)[0][0]] = -lp.sense * 0.5
    zeros = np.zeros(len(lp.a_value))
    kind, zero = "row 0 would change its kind", "no matrix nonzeros"
    return {"kind+zero": (dict(row_lower=lo, row_upper=up, a_value=zeros), kind),
            "zero+diagonal": (dict(a_value=zeros, q_value=q_bad), zero),
            "kind+diagonal": (dict(row_lower=lo, row_upper=up, q_value=q_bad), kind)}


def apply(lp, u):
    """The modified problem P' (a copy; the pattern arrays are shared)."""
    rest = {k: v for k, v in u.items() if k != "q_value"}
    out = MC.apply(lp, rest) if rest else copy.copy(lp)
    if u.get("q_value") is not None:
        out.hessian = (lp.hessian[0], lp.hessian[1], np.array(u["q_value"], dtype=np.float64))
    return out
