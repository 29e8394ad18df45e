"""tests/qp_setup_cases.py without a GPU: every maker sits on the edge it claims, counted by the host extraction
(pdlp_mi355x_host_prepare_qp) that both set-up paths share, and every broken problem is refused in the words the GPU test
expects."""
import numpy as np
import pytest

import qp_setup_cases as QC
from highs_amd import solver


def _nnz_off(lp, **options):
    return solver.host_prepare_qp(lp, **options)[1]["nnz_off"]


def test_tridiagonal_cases_straddle_one_block_of_the_scaling_kernel():
    slots = [_nnz_off(QC.tridiagonal_qp(q)) for q in QC.TRIDIAGONAL_COLUMNS]
    assert slots == [2, QC.SCALE_BLOCK - 2, QC.SCALE_BLOCK, QC.SCALE_BLOCK + 2]
    assert slots == [QC.off_diagonal_slots(QC.tridiagonal_qp(q)) for q in QC.TRIDIAGONAL_COLUMNS]
    lp = QC.tridiagonal_qp(128)
    form, hess = solver.host_prepare_qp(lp)
    assert len(lp.hessian[0]) - 1 == 128 < lp.num_col < form["n"]  # trailing columns and slack columns behind Q
    assert np.all(np.diff(hess["q_beg"])[128:] == 0)


def test_crafted_pattern_holds_what_it_lists():
    lp = QC.crafted_pattern_qp()
    st, idx, val = lp.hessian
    cols = np.repeat(np.arange(len(st) - 1), np.diff(st))
    pairs = list(zip(idx.tolist(), cols.tolist()))
    assert pairs.count((3, 0)) == 2 and pairs.count((4, 4)) == 2
    assert val[pairs.index((5, 1))] == 0.0 and val[pairs.index((2, 2))] == 0.0
    assert idx[st[3] + 1:st[4]].tolist() == [9, 6, 4]
    assert st[6] == st[7] and idx[st[5]:st[6]].tolist() == [5]
    plain, kept = _nnz_off(lp), _nnz_off(lp, updatable="hessian")
    assert (plain, kept) == (QC.off_diagonal_slots(lp), QC.off_diagonal_slots(lp, kept=True)) and kept == plain + 2


def test_dense_block_has_rows_of_599_entries():
    _, hess = solver.host_prepare_qp(QC.dense_block_qp())
    assert np.diff(hess["q_beg"]).max() == 599


@pytest.mark.parametrize("what", sorted(QC.REFUSALS))
def test_broken_hessians_are_refused_by_the_extraction(what):
    with pytest.raises(RuntimeError) as e:
        solver.host_prepare_qp(QC.refused(what))
    assert QC.REFUSALS[what] in str(e.value)
