"""Generated problems that sit exactly on the structural thresholds where the kernels change path, for
tests/test_edge_cases_host.py and tests/test_gpu_edges.py: fixed seeds, nothing read from disk.  Only `<=` rows and
bounded columns, so that formulation adds no slack column and keeps the order of rows and columns: major r of the
prepared A is row r here, major j of A' is column j.

values = "real": standard-normal coefficients.  values = "integer": coefficients drawn from the nonzero integers in
[-8, 8] — for runs without scaling (pdlp_features_off = 1) with an integer test vector in [-1024, 1024]: every product and
every partial sum, in any order, is then an exact double far below 2^53."""
import math

import numpy as np

from highs_amd import lp as L

INF = float("inf")


def _coefficients(rng, k, values):
    if values == "integer":
        v = rng.integers(1, 9, size=k).astype(np.float64)
        return v * rng.choice([-1.0, 1.0], size=k)
    assert values == "real", values
    return rng.standard_normal(k)


def _lp_from_rows(name, n, rows, rng, values):
    """rows: one sorted array of column indices per row.  Columns in [0, 1] with a nonzero cost, rows `<=` with a right-hand
    side taken from an interior point (a positive slack on every row, empty ones included)."""
    m = len(rows)
    lens = np.array([len(r) for r in rows], dtype=np.int64)
    r_start = np.concatenate([[0], np.cumsum(lens)])
    r_index = np.concatenate([np.asarray(r, dtype=np.int64) for r in rows] + [np.zeros(0, np.int64)])
    r_value = _coefficients(rng, int(r_start[-1]), values)
    cost = rng.standard_normal(n)
    cost[cost == 0.0] = 1.0
    x0 = rng.uniform(0.2, 0.8, n)
    act = np.zeros(m)
    np.add.at(act, np.repeat(np.arange(m), lens), r_value * x0[r_index])
    lp = L.HighsLp.from_rowwise(n, m, r_start, r_index, r_value, col_cost=cost, col_lower=np.zeros(n), col_upper=np.ones(n),
                                row_lower=np.full(m, -INF), row_upper=act + rng.uniform(0.1, 1.0, m))
    lp.model_name = name
    return lp


def _pick(rng, pool, k):
    return np.sort(rng.choice(pool, size=k, replace=False))


def limit_rows(chunk):
    """Lengths of the first ten rows of majors_at_limit(chunk)."""
    return (0, 1, 255, 257, 256, 1, chunk - 1, chunk + 1, chunk, 3)


def majors_at_limit(chunk, values="real", seed=11):
    """One operand whose rows have chunk - 1, chunk and chunk + 1 entries (chunk = 512: fewer than 2^18 nonzeros; 2048: filler
    rows of 60-70 entries bring it to 2^18), and 255 / 256 / 257 for the slab layout's limit, next to rows of 0 and 1 entries.
    Row order: empty, 1, 255, 257, 256, 1, chunk - 1, chunk + 1, chunk, 3, then the filler rows, last an empty one: every long
    row lies directly between two short ones.  Columns 1, 2, 3 hold chunk - 1, chunk + 1 and chunk entries (in the first
    filler rows), column 0 and the last column are empty, so the transposed operand sits on the same limits."""
    assert chunk in (512, 2048)
    rng = np.random.default_rng(seed + chunk)
    n = chunk + 160
    ordinary = np.arange(4, n - 1)  # (not the three tall columns, not the two empty ones)
    rows = [_pick(rng, ordinary, k) for k in limit_rows(chunk)]
    tall = {1: chunk - 1, 2: chunk + 1, 3: chunk}
    filler, nnz = 0, sum(len(r) for r in rows)
    while filler < chunk + 1 or (chunk == 2048 and nnz < 2**18):
        own = [c for c, k in tall.items() if filler < k]
        k = int(rng.integers(60, 71)) if chunk == 2048 else int(rng.integers(0, 5))
        rows.append(np.concatenate([np.array(own, dtype=np.int64), _pick(rng, ordinary, k)]))
        nnz += len(rows[-1])
        filler += 1
    rows.append(np.zeros(0, np.int64))
    return _lp_from_rows("limit%d" % chunk, n, rows, rng, values)


SEGMENT_ROWS = (513, 1025, 1025, 2048, 2049, 32768, 32769)


def segments(values="real", seed=13):
    """A chunk-512 operand (72 203 nonzeros) with consecutive long rows of 513, 1025, 1025, 2048, 2049 entries — 2, 3, 3, 4, 5
    segment tasks for workgroups of 4: contained in one workgroup; contained behind two idle tasks; contained behind one;
    contained, filling a workgroup behind one idle task; spanning — then 32768 (64 segments of 512, the most) and 32769
    entries (33 segments of 1024).  A short row before, two after."""
    rng = np.random.default_rng(seed)
    n = 33000
    cols = np.arange(n)
    rows = [_pick(rng, cols, 4)] + [_pick(rng, cols, k) for k in SEGMENT_ROWS] + [_pick(rng, cols, 1), _pick(rng, cols, 1)]
    return _lp_from_rows("segments", n, rows, rng, values)


def many_long(k, values="real", seed=17):
    """k rows of 257 entries (long in the slab layout, whose limit is 256) on 4096 columns, then 24 short rows; no column
    reaches 256 entries.  kLongSlotCap = 2048 such rows have a contribution slot each; 2049 share slots in groups of two."""
    rng = np.random.default_rng(seed)
    n = 4096
    rows = [np.sort(rng.permutation(n)[:257]) for _ in range(k)]
    rows += [_pick(rng, np.arange(n), int(rng.integers(0, 20))) for _ in range(24)]
    return _lp_from_rows("long%d" % k, n, rows, rng, values)


def empty_runs(values="real", seed=19, long_row=2500):
    """6000 rows, 6000 columns, 518 nonzeros: row 0 has 3 entries, row 2500 has 512 (columns 0 .. 511), row 2501 has 1, the
    last row has 2 (the last two columns), every other row is empty.  Work blocks hold at most 2048 majors:
      A   rows [0, 2048) with 3 entries | [2048, 2501) with 512 | [2501, 4549) with 1 | [4549, 6000) with 2
      A'  columns [0, 508) with 512 entries | [508, 2556) with 6 | [2556, 4604) with NONE | [4604, 6000) with 2
    long_row = 4600 (the 512 entries in row 4600, the single one in row 4601) gives A a block without entries too:
      A   rows [0, 2048) with 3 entries | [2048, 4096) with NONE | [4096, 4601) with 512 | [4601, 6000) with 3
    (the planner's own answer is asserted in tests/test_edge_cases_host.py)."""
    rng = np.random.default_rng(seed)
    n = m = 6000
    rows = [np.zeros(0, np.int64)] * m
    rows[0] = np.array([0, 1, 2])
    rows[long_row] = np.arange(512)
    rows[long_row + 1] = np.array([5])
    rows[m - 1] = np.array([n - 2, n - 1])
    return _lp_from_rows("empty_runs" if long_row == 2500 else "empty_runs%d" % long_row, n, rows, rng, values)


GRID_SHAPES = {32: (32, 512), 33: (33, 495), 64: (64, 512), 65: (65, 455)}


def grid(g, values="real", seed=23):
    """A dense LP whose two operands have exactly g work blocks of 512 entries each: a row of A is one block (n <= 512),
    512 // m columns of A' are one."""
    m, n = GRID_SHAPES[g]
    rng = np.random.default_rng(seed + g)
    return _lp_from_rows("grid%d" % g, n, [np.arange(n)] * m, rng, values)


def wide(n, values="real", seed=29):
    """4 rows of 500 entries that share no column, all on the first 2000 columns; every other column is empty, with a nonzero
    cost and finite bounds, so that its step matters.  A has 4 blocks, A' 8 / 11 / 11 for n = 10000 / 16384 / 16385: the
    ceil(n / 256) = 40 / 64 / 65 workgroups of the column step exceed both, the grid follows them up to 64, and at 16385
    column 16384 alone is left to the strided second pass of the column loop."""
    rng = np.random.default_rng(seed)  # (the same four rows for every n)
    perm = rng.permutation(2000)
    rows = [np.sort(perm[500 * i:500 * (i + 1)]) for i in range(4)]
    return _lp_from_rows("wide%d" % n, n, rows, np.random.default_rng(seed + n), values)


def arrow_qp(k, values="real", seed=9, n=700):
    """qp_small_cases.arrow_hessian(700) with only the first k off-diagonal entries of row / column 0 kept.  N (off-diagonal
    part, both triangles) then has one major of k entries, k majors of one entry and 699 - k empty majors.  k = 512: the
    longest major fills a 512-entry work block exactly; the 512 single entries fill a second one, which the 187 empty majors
    behind them join.  k = 513: a long major.
    Its two rows have 700 entries each — long majors of A, which alone would leave A without a work block, and the persistent
    loop takes no operand without one — so a third, short row (x_1 + x_2 <= 0.08) is added: what decides then is N.
    n = 4200 (the same construction on more columns): the block of the single entries is capped at 2048 majors, [1, 2049), and
    majors [2049, 4097) form a block of N WITHOUT entries."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.01, 0.05, n - 1)
    diag = np.concatenate([[1.0 + float(np.sum(b))], rng.uniform(0.2, 1.0, n - 1)])
    mu = rng.uniform(0.01, 0.15, n)
    second = rng.uniform(0.5, 1.5, n) if values == "real" else _coefficients(rng, n, values)
    A = np.vstack([np.ones(n), second, np.zeros(n)])
    A[2, 1:3] = 1.0
    cols, rws = np.nonzero(A.T)
    a_start = np.zeros(n + 1, np.int32)
    a_start[1:] = np.cumsum(np.bincount(cols, minlength=n))
    lp = L.HighsLp(n, 3, -mu, np.zeros(n), np.full(n, 0.05), np.array([1.0, 0.9, -INF]), np.array([1.0, INF, 0.08]), a_start,
                   rws.astype(np.int32), A[rws, cols], 1, 0.0, "arrow%d_%d" % (n, k)).normalise()
    # lower triangle, column-wise: column 0 holds the diagonal entry and the k kept entries, every other column its diagonal
    q_start = np.concatenate([[0], k + 1 + np.arange(n)]).astype(np.int32)
    q_index = np.concatenate([np.arange(k + 1), np.arange(1, n)]).astype(np.int32)
    q_value = np.concatenate([[diag[0]], b[:k], diag[1:]])
    lp.hessian = (q_start, q_index, q_value)
    return lp


# The whole-solve cases of tests/test_gpu_edges.py: name -> (maker, iteration cap).  Every cap was picked with the oracle
# alone so that the capped run holds a rejected trial and a restart (asserted in tests/test_edge_cases_host.py).
SOLVES = {
    "grid32": (lambda: grid(32), 1000), "grid33": (lambda: grid(33), 1000), "grid64": (lambda: grid(64), 1000),
    "grid65": (lambda: grid(65), 1000), "wide10000": (lambda: wide(10000), 1000), "wide16384": (lambda: wide(16384), 1000),
    "wide16385": (lambda: wide(16385), 1000), "empty_runs": (empty_runs, 400), "empty_runs4600": (lambda: empty_runs(long_row=4600), 400),
    "arrow512": (lambda: arrow_qp(512), 400), "arrow513": (lambda: arrow_qp(513), 400),
    "arrow512n4200": (lambda: arrow_qp(512, n=4200), 400),
}


# ---- a reference that depends on no summation order -----------------------------------------------------------------------
def two_prod(a, b):
    """Dekker's product: (p, e) with p = fl(a b) and p + e = a b exactly (Veltkamp splitting; no overflow or underflow at the
    magnitudes of these cases)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    p = a * b
    ca, cb = 134217729.0 * a, 134217729.0 * b
    ah, bh = ca - (ca - a), cb - (cb - b)
    al, bl = a - ah, b - bh
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


def exact_major_sums(beg, idx, val, x):
    """Per major of a compressed matrix: (the exact sum of its products val * x[idx], rounded once — math.fsum over both halves
    of every exact product; sum of |product|; entries).  Nothing here depends on the order of the entries."""
    p, e = two_prod(val, np.asarray(x)[idx])
    a = np.abs(p)
    m = len(beg) - 1
    exact, scale = np.zeros(m), np.zeros(m)
    for r in range(m):
        b0, b1 = beg[r], beg[r + 1]
        if b1 > b0:
            exact[r] = math.fsum(np.concatenate([p[b0:b1], e[b0:b1]]))
            scale[r] = math.fsum(a[b0:b1])
    return exact, scale, np.diff(beg)
