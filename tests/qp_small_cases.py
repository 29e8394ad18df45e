"""Generated small QPs with off-diagonal Hessian entries for tests/test_gpu_qp_small.py and tools/qp_small_bench.py: fixed
seeds, so that every caller sees the same problem."""
import numpy as np

from highs_amd import lp as L


def _colwise(A):
    """Dense row-major matrix -> (a_start, a_index, a_value), entries of a column in ascending row order."""
    m, n = A.shape
    cols, rows = np.nonzero(A.T)
    a_start = np.zeros(n + 1, np.int32)
    a_start[1:] = np.cumsum(np.bincount(cols, minlength=n))
    return a_start, rows.astype(np.int32), A[rows, cols]


def portfolio(n=64, seed=7, factors=6):
    """Markowitz with a dense covariance: min 1/2 x'Qx - mu'x, sum x = 1, a'x >= r, 0 <= x <= 0.2.  Q = F F' + diag is
    dense PSD, so N has n (n - 1) entries — for n = 64, 4032 = 8 work blocks of 8 rows — and A has two rows (one block):
    the grid of the persistent loop is set by N."""
    rng = np.random.default_rng(seed)
    F = rng.standard_normal((n, factors)) * 0.3
    Q = F @ F.T + np.diag(rng.uniform(0.05, 0.3, n))
    mu = rng.uniform(0.01, 0.15, n)
    a = rng.uniform(0.5, 1.5, n)
    A = np.vstack([np.ones(n), a])
    st, idx, val = _colwise(A)
    inf = float("inf")
    lp = L.HighsLp(n, 2, -mu, np.zeros(n), np.full(n, 0.2), np.array([1.0, 0.9]), np.array([1.0, inf]), st, idx, val, 1, 0.0,
                   "portfolio%d" % n).normalise()
    return lp.set_hessian_from_dense(Q)


def dense_hessian(n=600, seed=5):
    """The same shape with a dense Q on 600 columns: every row of N has 599 entries, more than a 512-entry work block."""
    lp = portfolio(n, seed, factors=4)
    lp.col_upper = np.full(n, 0.05)
    lp.model_name = "dense%d" % n
    return lp


def arrow_hessian(n=700, seed=9):
    """Q = diag + one dense row / column (a common factor every asset loads on): N has 2 (n - 1) entries — 512-entry work
    blocks — and ONE row of n - 1 = 699 entries: a long major."""
    rng = np.random.default_rng(seed)
    b = rng.uniform(0.01, 0.05, n - 1)
    Q = np.diag(np.concatenate([[1.0 + float(np.sum(b))], rng.uniform(0.2, 1.0, n - 1)]))
    Q[1:, 0] = b
    Q[0, 1:] = b
    mu = rng.uniform(0.01, 0.15, n)
    A = np.vstack([np.ones(n), rng.uniform(0.5, 1.5, n)])
    st, idx, val = _colwise(A)
    inf = float("inf")
    lp = L.HighsLp(n, 2, -mu, np.zeros(n), np.full(n, 0.05), np.array([1.0, 0.9]), np.array([1.0, inf]), st, idx, val, 1, 0.0,
                   "arrow%d" % n).normalise()
    return lp.set_hessian_from_dense(Q)


def mpc(horizon=40, nx=4, nu=2, seed=3):
    """A linear MPC horizon: states x_t and inputs u_t, dynamics x_{t+1} = A x_t + B u_t as equality rows (block-banded
    matrix), stage cost 1/2 (x_t' Qx x_t + u_t' R u_t) with coupled states and a rate term (u_t - u_{t-1})' S (u_t - u_{t-1})
    that links neighbouring stages (block-tridiagonal Hessian), box bounds.  A few thousand nonzeros."""
    rng = np.random.default_rng(seed)
    Ad = np.eye(nx) + 0.1 * rng.standard_normal((nx, nx))
    Bd = 0.3 * rng.standard_normal((nx, nu))
    G = rng.standard_normal((nx, nx))
    Qx = G @ G.T / nx + 0.1 * np.eye(nx)
    H = rng.standard_normal((nu, nu))
    Ru = H @ H.T / nu + 0.1 * np.eye(nu)
    S = 0.5 * np.eye(nu)
    per = nx + nu
    n = horizon * per
    m = horizon * nx
    A = np.zeros((m, n))
    Q = np.zeros((n, n))
    x0 = rng.uniform(-1.0, 1.0, nx)
    rl = np.zeros(m)
    for t in range(horizon):
        xs, us = t * per, t * per + nx  # x_{t+1} and u_t of stage t
        r = t * nx
        A[r:r + nx, xs:xs + nx] = np.eye(nx)
        A[r:r + nx, us:us + nu] = -Bd
        if t > 0:
            A[r:r + nx, xs - per:xs - per + nx] = -Ad
        else:
            rl[r:r + nx] = Ad @ x0
        Q[xs:xs + nx, xs:xs + nx] += Qx
        Q[us:us + nu, us:us + nu] += Ru + S
        if t > 0:
            Q[us:us + nu, us:us + nu] += S
            Q[us:us + nu, us - per:us - per + nu] -= S
            Q[us - per:us - per + nu, us:us + nu] -= S
    lo = np.tile(np.concatenate([np.full(nx, -5.0), np.full(nu, -1.0)]), horizon)
    st, idx, val = _colwise(A)
    lp = L.HighsLp(n, m, np.zeros(n), lo, -lo, rl, rl.copy(), st, idx, val, 1, 0.0, "mpc%d" % horizon).normalise()
    return lp.set_hessian_from_dense(Q)
