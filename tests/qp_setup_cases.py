"""QPs whose Hessian has an off-diagonal part, for tests/test_gpu_qp_setup_device.py: the goldens and generated problems the
other QP tests use, and small patterns that sit on the edges of the device-side set-up of N — slot counts around one
256-thread block of the kernel that scales N inside the passes, rows of N long enough for segment tasks, empty rows behind
q_dim, and the pattern contract's corner cases (repeated pairs, explicit zeros, descending rows).  Makers only; every one
returns a fresh HighsLp."""
import os

import numpy as np

import lpgen
from highs_amd import lp as L
from highs_amd import solver

GOLD = os.path.join(os.path.dirname(__file__), "golden")
GOLDENS = ("sq0", "sq3", "sq100", "qjh_mps")
SCALE_BLOCK = 256  # threads per block of the kernel that scales N's slots (pdlp_setup.hip kT)
# columns in Q -> 2 (q - 1) off-diagonal slots of a tridiagonal Q: one pair, one below / at / above one block
TRIDIAGONAL_COLUMNS = (2, 128, 129, 130)


def golden(name):
    return L.HighsLp.from_npz(os.path.join(GOLD, "qp", name + ".npz"))


def dense_block_qp():
    """2 000 columns, Q = diag(d) + beta beta' on 600 of them: every row of N in that block has 599 entries, so the N
    operand has long majors and segment tasks (as tests/test_gpu_update_hessian.py's, restated)."""
    lp = lpgen.drop_free_rows(lpgen.random_lp(4, m=40, n=2000))
    rng = np.random.default_rng(17)
    n = lp.num_col
    block = np.sort(rng.choice(n, 600, replace=False))
    beta = np.zeros(n)
    beta[block] = rng.uniform(0.2, 1.0, 600) * rng.choice([-1.0, 1.0], 600)
    Q = np.outer(beta, beta) + np.diag(rng.uniform(0.1, 2.0, n))
    return lp.set_hessian_from_dense(lp.sense * Q)


def tridiagonal_hessian(q_dim, seed, sense=1):
    """(start, index, value) of a diagonally dominant tridiagonal Q on the first q_dim columns: 2 (q_dim - 1) off-diagonal
    slots of N."""
    rng = np.random.default_rng(seed)
    off = rng.uniform(-0.5, 0.5, q_dim - 1)
    off = np.where(off == 0.0, 0.25, off)
    diag = np.abs(np.concatenate([off, [0.0]])) + np.abs(np.concatenate([[0.0], off])) + rng.uniform(0.0, 1.0, q_dim)
    st = np.zeros(q_dim + 1, np.int32)
    st[1:] = np.cumsum(np.concatenate([np.full(q_dim - 1, 2), [1]]))
    idx = np.empty(2 * q_dim - 1, np.int32)
    val = np.empty(2 * q_dim - 1)
    idx[0::2] = np.arange(q_dim); val[0::2] = diag
    idx[1::2] = np.arange(1, q_dim); val[1::2] = off
    return st, idx, sense * val


def tridiagonal_qp(q_cols):
    """A small random LP (ranged and free rows: slack columns behind the caller's) with a tridiagonal Q on its first q_cols
    columns.  q_cols = 128 and 2 leave trailing columns outside Q (q_dim < num_col): their rows of N, and those of every
    slack column, are empty."""
    num_col = {2: 6, 128: 131}.get(q_cols, q_cols)
    lp = lpgen.random_lp(8, m=14, n=num_col)  # (seed 8: minimisation, no emptied row or column)
    lp.hessian = tridiagonal_hessian(q_cols, 40 + q_cols, lp.sense)
    return lp


def crafted_pattern_qp():
    """12 columns; the lower triangle column by column holds a repeated (row, column) pair, an explicit 0.0 off the diagonal
    and one on it, a column whose rows come in descending order, a column with only a diagonal slot, a column with no slot
    and a repeated diagonal slot.  Diagonally dominant, so positive semidefinite.  A plain solver drops the zeros; a
    Hessian-updatable one keeps them as slots."""
    n = 12
    lp = lpgen.random_lp(4, m=8, n=n)  # (seed 4: minimisation, no emptied row or column)
    off = {0: [(3, 0.4), (3, -0.15)],           # the pair (3, 0) twice
           1: [(5, 0.0)],                        # an explicit zero off the diagonal
           3: [(9, 0.3), (6, -0.2), (4, 0.35)],  # descending rows
           7: [(8, -0.45)], 8: [(11, 0.25)], 10: [(11, -0.3)]}
    dom = np.zeros(n)
    for j, entries in off.items():
        for i, v in entries:
            dom[i] += abs(v); dom[j] += abs(v)
    diag = dom + 0.5 + 0.1 * np.arange(n)
    st, idx, val = [0], [], []
    for j in range(n):
        if j == 2:
            idx += [2]; val += [0.0]                                # an explicit zero on the diagonal, nothing else
        elif j == 4:
            idx += [4, 4]; val += [0.75 * diag[4], 0.25 * diag[4]]  # a repeated diagonal slot
        elif j == 6:
            pass                                                    # no slot at all
        else:
            idx += [j]; val += [diag[j]]                            # (5, 9 and 11: a diagonal slot only)
            for i, v in off.get(j, []):
                idx.append(i); val.append(v)
        st.append(len(idx))
    lp.hessian = (np.array(st, np.int32), np.array(idx, np.int32), lp.sense * np.array(val))
    return lp


def large_tridiagonal_qp():
    """The 40 000 x 40 000 random sparse LP (320 000 nonzeros: above the 200 000 of the automatic rule) with the tridiagonal
    Hessian of tests/test_gpu_qp.py's large sparse-Hessian case, restated."""
    sp_ = solver.SyntheticProblem(40000, 40000, 320000, 3)
    lp = sp_.to_lp()
    sp_.close()
    n = lp.num_col
    rng = np.random.default_rng(11)
    off = rng.uniform(-0.5, 0.5, n - 1)
    diag = np.abs(np.concatenate([off, [0.0]])) + np.abs(np.concatenate([[0.0], off])) + rng.uniform(0.0, 1.0, n)
    st = np.zeros(n + 1, np.int32)
    st[1:] = np.cumsum(np.concatenate([np.full(n - 1, 2), [1]]))
    idx = np.empty(2 * n - 1, np.int32); val = np.empty(2 * n - 1)
    idx[0::2] = np.arange(n); val[0::2] = diag
    idx[1::2] = np.arange(1, n); val[1::2] = off
    lp.hessian = (st, idx, val)
    return lp


# name -> maker; the seed random_sparse_qp was made with is SPARSE_SEED (update_hessian_cases.new_values redraws its G)
SPARSE_SEED = 3
CASES = {name: (lambda name=name: golden(name)) for name in GOLDENS}
CASES.update({
    "bench_qp_banded": lambda: lpgen.bench_qp_at_scale(200, True),
    "random_sparse_qp": lambda: lpgen.random_sparse_qp(SPARSE_SEED),  # sense = -1
    "dense_block": dense_block_qp,
    "crafted": crafted_pattern_qp,
})
CASES.update({"tridiagonal_%d" % q: (lambda q=q: tridiagonal_qp(q)) for q in TRIDIAGONAL_COLUMNS})


def off_diagonal_slots(lp, kept=False):
    """Slots of N as the extraction counts them: both triangles, repeated pairs merged; zero values dropped unless `kept`."""
    st, idx, val = lp.hessian
    cols = np.repeat(np.arange(len(st) - 1), np.diff(st))
    sel = (idx != cols) & (kept | (np.asarray(val) != 0.0))
    return 2 * len(set(zip(np.asarray(idx)[sel].tolist(), cols[sel].tolist())))


# ---- refusals: name -> (maker of the broken problem, words of the refusal) ---------------------------------------------------
def _broken(what):
    lp = crafted_pattern_qp()
    st, idx, val = (np.array(a) for a in lp.hessian)
    if what == "upper_triangle":
        idx[st[7] + 1] = 5  # (8, 7) -> (5, 7)
    elif what == "index_out_of_range":
        idx[st[7] + 1] = lp.num_col
    elif what == "negative_diagonal":
        val[st[4] + 1] = -2.0 * val[st[4]]  # the two slots of (4, 4) add up to a negative number
    elif what == "q_dim_above_num_col":
        st = np.concatenate([st, st[-1:]]).astype(np.int32)
    lp.hessian = (st.astype(np.int32), idx.astype(np.int32), val)
    return lp


REFUSALS = {
    "upper_triangle": "lower triangle",
    "index_out_of_range": "Hessian index out of range",
    "negative_diagonal": "not positive semidefinite",
    "q_dim_above_num_col": "Hessian dimension exceeds the number of columns",
}


def refused(what):
    return _broken(what)
