"""The Hessian's extraction restated in numpy, the way the device does it (highs_amd/csrc/pdlp_setup.hip
gpuExtractHessian): every taken off-diagonal slot (i, j) gives a head entry (row i, column j) and a tail entry (row j,
column i); all heads in slot order, then all tails, sorted stably by column and then stably by row; a run of equal (row,
column) is one slot of N.  tests/test_hessian_extraction_host.py holds this against the host walk (pdlp_host.cpp), the GPU
test holds the device's kept map against it.  A helper, not a conftest."""
import numpy as np


def extraction(lp, n, kept):
    """lp.hessian -> dict: the assembly map (dst_beg [n + n_off + 1], src_slot, off_row, off_col), N's row starts q_beg
    [n + 1], and qdiag [n] / q_val [n_off] assembled with lp.sense in the walk's order of additions; taken = slots taken.
    n: columns of the formulated problem (slack columns included).  q_start must run from 0 upwards."""
    st, idx, val = (np.asarray(a) for a in lp.hessian)
    q_dim, nq = len(st) - 1, int(st[-1])
    assert st[0] == 0 and np.all(np.diff(st) >= 0)
    idx, val = idx[:nq].astype(np.int64), val[:nq].astype(np.float64)
    col = np.repeat(np.arange(q_dim, dtype=np.int64), np.diff(st))
    slot = np.arange(nq, dtype=np.int64)
    taken = np.ones(nq, bool) if kept else ~(val == 0.0)  # (== 0.0 drops -0.0 and keeps a NaN)
    diag, off = taken & (idx == col), taken & (idx != col)
    dcnt = int(diag.sum())
    diag_beg = np.concatenate([[0], np.cumsum(np.bincount(col[diag], minlength=n))])
    p = slot[off]
    row_e, col_e, src_e = np.concatenate([idx[p], col[p]]), np.concatenate([col[p], idx[p]]), np.concatenate([p, p])
    for key in ("col", "row"):
        order = np.argsort(col_e if key == "col" else row_e, kind="stable")
        row_e, col_e, src_e = row_e[order], col_e[order], src_e[order]
    n_ent = len(src_e)
    head = np.ones(n_ent, bool)
    head[1:] = (row_e[1:] != row_e[:-1]) | (col_e[1:] != col_e[:-1])
    first = np.nonzero(head)[0]
    dst_beg = np.concatenate([diag_beg, dcnt + first[1:], [dcnt + n_ent] if n_ent else []]).astype(np.int64)
    src_slot = np.concatenate([slot[diag], src_e])
    off_row, off_col = row_e[first], col_e[first]
    # values: a source times the sense; the diagonal summed from 0.0, a slot of N from its first source, left to right
    prod = val[src_slot] * float(lp.sense)
    n_dst = len(dst_beg) - 1
    out = np.zeros(n_dst)
    lens = np.diff(dst_beg)
    one = lens == 1
    out[one] = prod[dst_beg[:-1][one]]
    out[:n] = 0.0 + out[:n]  # (the diagonal starts from 0.0: a lone -0.0 becomes 0.0)
    for d in np.nonzero(lens > 1)[0]:
        b, e = dst_beg[d], dst_beg[d + 1]
        acc = 0.0 + prod[b] if d < n else prod[b]
        for k in range(b + 1, e):
            acc = acc + prod[k]
        out[d] = acc
    return dict(taken=int(taken.sum()), n_off=len(first), dst_beg=dst_beg, src_slot=src_slot, off_row=off_row, off_col=off_col,
                q_beg=np.searchsorted(off_row, np.arange(n + 1), side="left"), qdiag=out[:n], q_val=out[n:])
