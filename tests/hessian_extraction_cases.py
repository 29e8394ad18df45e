"""QPs for the Hessian's extraction (highs_amd/csrc/pdlp_setup.hip gpuExtractHessian against the host walk of
pdlp_host.cpp), for tests/test_hessian_extraction_host.py and tests/test_gpu_hessian_extraction.py: the problems of
tests/qp_setup_cases.py that sit on the extraction's edges, and small patterns for what those leave out — slot counts at one
256-thread block of the classification, repeated pairs inside a descending column, Hessians without a diagonal or without
anything else, zeros of both signs, empty border columns, and slots that only one of the two modes refuses.  Makers only;
every one returns a fresh HighsLp."""
import numpy as np

import lpgen
import qp_setup_cases as QC

BLOCK = 256  # threads per block of the extraction's kernels (pdlp_setup.hip kT)
NUM_COL = 12


def from_columns(columns, num_col=NUM_COL, q_dim=None):
    """A small random LP (seed 4: minimisation, no emptied row or column) whose Hessian holds, column by column in the given
    order, the slots `columns[j]` = [(row, value), ...]."""
    lp = lpgen.random_lp(4, m=8, n=num_col)
    q_dim = num_col if q_dim is None else q_dim
    st, idx, val = [0], [], []
    for j in range(q_dim):
        for i, v in columns.get(j, []):
            idx.append(i); val.append(v)
        st.append(len(idx))
    lp.hessian = (np.array(st, np.int32), np.array(idx, np.int32), lp.sense * np.array(val, np.float64))
    return lp


def _dominant(off, zero_columns=()):
    """columns of a diagonally dominant Q from its off-diagonal slots: a diagonal slot first in every column."""
    dom = np.zeros(NUM_COL)
    for j, entries in off.items():
        for i, v in entries:
            if 0 <= i < NUM_COL:
                dom[i] += abs(v); dom[j] += abs(v)
    return {j: ([] if j in zero_columns else [(j, dom[j] + 0.5 + 0.1 * j)]) + list(off.get(j, [])) for j in range(NUM_COL)}


BASE_OFF = {0: [(3, 0.4)], 1: [(4, -0.2), (9, 0.3)], 3: [(6, 0.25)], 5: [(7, -0.35), (10, 0.15)], 8: [(11, 0.2)]}


def slots_256_qp():
    """Exactly 256 caller slots: the 255 of the tridiagonal Q on 128 columns and a second slot of its last diagonal entry."""
    lp = QC.tridiagonal_qp(128)
    st, idx, val = (np.array(a) for a in lp.hessian)
    st[-1] += 1
    idx = np.concatenate([idx, [127]]).astype(np.int32)
    val = np.concatenate([val, [0.5 * lp.sense]])
    lp.hessian = (st.astype(np.int32), idx, val)
    assert len(val) == BLOCK
    return lp


def triple_pair_qp():
    """Column 1 comes in descending rows and holds the pair (5, 1) three times, with other rows between the repeats."""
    off = dict(BASE_OFF)
    off[1] = [(9, 0.2), (5, 0.1), (7, 0.3), (5, -0.05), (4, 0.25), (5, 0.15), (2, 0.1)]
    return from_columns(_dominant(off))


def diagonal_only_qp():
    cols = {j: [(j, 0.5 + 0.1 * j)] for j in range(NUM_COL)}
    cols[4] = [(4, 0.3), (4, 0.6)]
    del cols[6]
    return from_columns(cols)


def off_diagonal_only_qp():
    """No diagonal slot at all (the diagonal of Q is zero: the set-up accepts it, whatever the solve makes of it)."""
    return from_columns({0: [(3, 0.01)], 2: [(5, -0.02), (4, 0.01)], 7: [(8, 0.015)]})


def all_zero_qp():
    """Every value is 0.0: a plain solver has an LP, a Hessian-updatable one keeps the diagonal and N as slots of zeros."""
    cols = _dominant(BASE_OFF)
    return from_columns({j: [(i, 0.0) for i, _ in entries] for j, entries in cols.items()})


def negative_zero_qp():
    """An off-diagonal -0.0 (== 0.0: dropped by a plain solver like +0.0) and a diagonal one."""
    off = dict(BASE_OFF)
    off[1] = [(4, -0.2), (6, -0.0), (9, 0.3)]
    cols = _dominant(off)
    cols[2] = [(2, -0.0)]
    return from_columns(cols)


def empty_border_columns_qp():
    off = {j: e for j, e in BASE_OFF.items() if j != 0}
    return from_columns(_dominant(off, zero_columns=(0, NUM_COL - 1)))


def zero_above_diagonal_qp():
    """(2, 5) lies above the diagonal with the value 0.0: a plain solver never looks at it, a Hessian-updatable one refuses."""
    off = dict(BASE_OFF)
    off[5] = [(7, -0.35), (2, 0.0), (10, 0.15)]
    return from_columns(_dominant(off))


def zero_out_of_range_qp():
    off = dict(BASE_OFF)
    off[5] = [(7, -0.35), (NUM_COL, 0.0), (10, 0.15)]
    return from_columns(_dominant(off))


def two_offenders_qp(first):
    """A slot above the diagonal and a slot out of range, both non-zero, `first` ("above" / "range") in the earlier column."""
    off = dict(BASE_OFF)
    above, outside = (1, 0.2), (-1, 0.2)
    off[3] = [(6, 0.25), above if first == "above" else outside]
    off[8] = [(11, 0.2), outside if first == "above" else above]
    return from_columns(_dominant(off))


def decreasing_start_qp():
    """q_start = [0, 2, 1, 3]: it decreases once, so column 1 is empty and slot 1 belongs to column 0 as (2, 0) and to column 2
    as a second (2, 2).  The host walk accepts it; the device extraction leaves such starts to the walk."""
    lp = lpgen.random_lp(4, m=8, n=NUM_COL)
    lp.hessian = (np.array([0, 2, 1, 3], np.int32), np.array([0, 2, 2], np.int32), lp.sense * np.array([1.0, 0.3, 1.0]))
    return lp


# name -> maker: what both modes accept (all_zero, negative_zero: the modes differ in what they keep)
NEW_CASES = {
    "slots_256": slots_256_qp,
    "triple_pair": triple_pair_qp,
    "diagonal_only": diagonal_only_qp,
    "off_diagonal_only": off_diagonal_only_qp,
    "all_zero": all_zero_qp,
    "negative_zero": negative_zero_qp,
    "empty_border_columns": empty_border_columns_qp,
}
SETUP_CASES = ("crafted", "tridiagonal_2", "tridiagonal_128", "tridiagonal_129", "tridiagonal_130", "dense_block", "random_sparse_qp",
               "sq100")
CASES = {name: QC.CASES[name] for name in SETUP_CASES}
CASES.update(NEW_CASES)
CASES["large_tridiagonal"] = QC.large_tridiagonal_qp

# name -> (maker, words of the refusal, modes that refuse: "plain" = a plain solver, "kept" = updatable="hessian")
REFUSALS = {name: ((lambda name=name: QC.refused(name)), words, ("plain", "kept")) for name, words in QC.REFUSALS.items()}
REFUSALS.update({
    "zero_above_diagonal": (zero_above_diagonal_qp, "(entry (2,5) lies above the diagonal)", ("kept",)),
    "zero_out_of_range": (zero_out_of_range_qp, "Hessian index out of range", ("plain", "kept")),
    "above_then_range": (lambda: two_offenders_qp("above"), "(entry (1,3) lies above the diagonal)", ("plain", "kept")),
    "range_then_above": (lambda: two_offenders_qp("range"), "Hessian index out of range", ("plain", "kept")),
})


def caller_slots(lp):
    return int(lp.hessian[0][-1])
