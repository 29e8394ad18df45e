"""Seeded changes of the matrix VALUES of an LP / QP on its fixed sparsity pattern, as pdlp_mi355x_update_matrix takes
them, for tests/test_update_matrix_host.py and tests/test_gpu_update_matrix.py.  `new_values` returns a_value in the
positions of lp.a_value; `modification` returns the keyword arguments of DeviceSolver.update_matrix; `apply` builds the
modified problem P' in Python (a helper, not a conftest)."""
import copy

import numpy as np

import update_cases as UC

# the parts of a value change, applied in this order
PARTS = ("jitter", "decades", "signs", "zeros", "zero_row_col")
KINDS = PARTS + ("values", "all")  # "values": all parts together; "all": that with update_cases.modification(lp, "all")


def _rows_cols(lp):
    start = np.asarray(lp.a_start, dtype=np.int64)
    rows = np.asarray(lp.a_index, dtype=np.int64)
    cols = np.repeat(np.arange(lp.num_col, dtype=np.int64), np.diff(start))
    return rows, cols


def new_values(lp, seed, parts=PARTS):
    rng = np.random.default_rng(seed)
    a = np.array(lp.a_value, dtype=np.float64)
    nnz = a.size
    rows, cols = _rows_cols(lp)
    if "jitter" in parts:  # every value moves
        a = a * (1.0 + 0.3 * rng.standard_normal(nnz))
    if "decades" in parts:  # about 1/7 of the entries by powers of ten over +-3 decades: the Ruiz factors really move
        k = max(1, nnz // 7)
        at = rng.choice(nnz, k, replace=False)
        a[at] = a[at] * 10.0 ** rng.integers(-3, 4, k).astype(np.float64)
    if "signs" in parts:  # about 1/10 change their sign
        k = max(1, nnz // 10)
        at = rng.choice(nnz, k, replace=False)
        a[at] = -a[at]
    if "zeros" in parts:  # a few exact zeros (create keeps explicit zeros) ...
        k = max(1, min(max(2, nnz // 200), nnz // 4))
        a[rng.choice(nnz, k, replace=False)] = 0.0
        # ... one of them inside the longest column and one inside the longest row (a long major, where the LP has one)
        j = int(np.argmax(np.diff(np.asarray(lp.a_start, dtype=np.int64))))
        in_col = np.nonzero(cols == j)[0]
        a[in_col[in_col.size // 2]] = 0.0
        i = int(np.argmax(np.bincount(rows, minlength=lp.num_row)))
        in_row = np.nonzero(rows == i)[0]
        a[in_row[in_row.size // 2]] = 0.0
    if "zero_row_col" in parts:  # one whole row and one whole column: the `== 0 ? 1` branches of the scaling
        a[rows == rows[rng.integers(nnz)]] = 0.0
        a[cols == cols[rng.integers(nnz)]] = 0.0
    if not np.any(a != 0.0):  # (a 2 x 2 LP: an all-zero matrix is refused, by create too)
        a[0] = lp.a_value[0]
    return a


def modification(lp, what, seed):
    if what in PARTS:
        return dict(a_value=new_values(lp, seed, (what,)))
    u = dict(a_value=new_values(lp, seed))
    if what == "all":
        u.update(UC.modification(lp, "all", seed + 1))
    else:
        assert what == "values", what
    return u


def apply(lp, u):
    """The modified problem P' (a copy; the pattern arrays are shared)."""
    out = UC.apply(lp, {k: v for k, v in u.items() if k != "a_value"}) if len(u) > 1 else copy.copy(lp)
    if u.get("a_value") is not None:
        out.a_value = np.array(u["a_value"], dtype=np.float64)
    return out
