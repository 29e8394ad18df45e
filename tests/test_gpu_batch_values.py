"""pdlp_mi355x_batch_run_values on the device: every R[k] of a batch whose variants change matrix and Hessian VALUES must
be, bit for bit, what ONE held solver created with the batch's updatable bits gives for update_values / update_matrix /
update + run — every solution vector, count and scalar.  The references (batch_values_cases.reference) are code that
exists without this entry, computed before the batch call and shared.  Every value variant must really change the solve
(its reference differs from P's own), and a variant without arrays behind a value variant must give P's own result
exactly: a no-op implementation fails the first, a missing restore the second."""
import re

import numpy as np
import pytest

import batch_values_cases as BC
import update_hessian_cases as HC
from highs_amd import solver

pytestmark = pytest.mark.gpu
OPTIONS = BC.OPTIONS


def _references(name, updatable, tagged):
    refs = [BC.reference(name, updatable, t) for t in tagged]
    own = BC.reference(name, updatable, BC.NOTHING)[0]
    for (tag, v), (R, _) in zip(tagged, refs):
        limited = "iter_limit" in v or "start" in v
        if BC.has_values(v) and not limited:
            assert BC.really_differs(R, own), (name, tag, "the variant does not change the solve", R.num_iter)
    return refs


def _run_and_compare(name, updatable, batch, tagged):
    refs = _references(name, updatable, tagged)
    out = batch.run([v for _, v in tagged])
    assert len(out) == len(tagged)
    for (tag, _), o, (R, _) in zip(tagged, out, refs):
        assert BC.same_result(o.result, R) is None, (name, tag, BC.same_result(o.result, R))
    return batch.info(), refs


def _launch_bounds(I, refs):
    """test_gpu_batch.py's bounds for a run in which nothing is refilled"""
    solo = [r[1] for r in refs]
    assert I.trial_launches <= max(solo) + 15, (I.trial_launches, solo)
    assert I.check_launches == I.trial_launches + 1


# ---- 1: an LP's matrix values ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [8, 11])
def test_lp_matrix_values_on_eight_lanes(K):
    name = "adlittle"
    kinds = ["jitter", "decades", "signs", "zeros", "values", "all", "zero_row_col", "jitter"]
    tagged = [BC.matrix(name, what, 31 + i) for i, what in enumerate(kinds)]
    if K == 11:  # the refills: a data variant and P itself behind value variants, and a value variant behind those
        tagged = tagged[:6] + [BC.data(name, "cost", 5), BC.NOTHING] + tagged[6:] + [BC.matrix(name, "values", 47)]
    assert len(tagged) == K
    batch = solver.DeviceBatch(BC.lp(name), lanes=8, updatable="matrix", **OPTIONS)
    I, refs = _run_and_compare(name, "matrix", batch, tagged)
    batch.close()
    print("batch info:", I.text, I.lanes_concurrent, I.trial_launches, I.check_launches, [r[1] for r in refs])
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (8, 8, K, 0), I.text
    if K == 8:
        _launch_bounds(I, refs)


# ---- 2: an off-diagonal QP's Hessian values -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["sq100", "portfolio64"])
def test_qp_hessian_values_sweep_then_a_mix(name):
    updatable = "matrix+hessian"
    # (a portfolio's two rows are its budget and its return: only a jitter leaves it a portfolio)
    a_kind = "jitter" if name == "portfolio64" else "values"
    sweep = [BC.hessian(name, "scale" + f) for f in ("0.3", "0.5", "2", "3", "5", "7", "0.1")] + [BC.hessian(name, "regen", 41)]
    batch = solver.DeviceBatch(BC.lp(name), lanes=8, updatable=updatable, **OPTIONS)
    I, refs = _run_and_compare(name, updatable, batch, sweep)
    print("sweep info:", I.text, I.lanes_concurrent, I.trial_launches, I.check_launches, [r[1] for r in refs])
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (8, 8, 8, 0), I.text
    assert I.text.startswith("concurrent: 8 lanes"), I.text
    _launch_bounds(I, refs)
    mix = [BC.hessian(name, "scale7"), BC.matrix(name, a_kind, 43), BC.both(name, a_kind, "regen", 44), BC.data(name, "cost", 5),
           BC.NOTHING, BC.hessian(name, "regen", 46), BC.NOTHING, BC.matrix(name, "jitter", 47), BC.data(name, "all", 6),
           BC.both(name, "jitter", "scale0.3", 48), BC.NOTHING]
    I, refs = _run_and_compare(name, updatable, batch, mix)
    batch.close()
    assert (I.lanes_concurrent, I.variants, I.fallback_variants) == (8, 11, 0), I.text


# ---- 3: every restore transition, deterministically ---------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [1, 2])
def test_every_restore_transition(lanes):
    """One lane: the sequential loop through the lane's own update, so that every variant follows the one before it:
    [A, none, Q, none, A+Q, data, Q, none] — P after A, P after Q, data alone after A+Q (both go back), Q after data (the
    data go back), P after Q."""
    name, updatable = "sq100", "matrix+hessian"
    tagged = [BC.matrix(name, "values", 51), BC.NOTHING, BC.hessian(name, "scale7"), BC.NOTHING, BC.both(name, "values", "regen", 52),
              BC.data(name, "all", 7), BC.hessian(name, "regen", 54), BC.NOTHING]
    batch = solver.DeviceBatch(BC.lp(name), lanes=lanes, updatable=updatable, **OPTIONS)
    I, _ = _run_and_compare(name, updatable, batch, tagged)
    if lanes == 1:
        assert (I.lanes_concurrent, I.trial_launches, I.text) == (1, 0, "sequential: one lane")
    else:
        assert (I.lanes_concurrent, I.fallback_variants) == (2, 0), I.text
    # and the same list once more on the lanes as the first run left them
    _run_and_compare(name, updatable, batch, tagged[::-1])
    batch.close()


# ---- 4: a diagonal QP with the matrix bit only: the update_matrix path -----------------------------------------------------------
def test_diagonal_qp_matrix_values_take_update_matrix():
    name, updatable = "qp0", "matrix"
    tagged = [BC.matrix(name, "values", 61), BC.NOTHING, BC.matrix(name, "all", 62), BC.matrix(name, "jitter", 63), BC.data(name, "cost", 8)]
    batch = solver.DeviceBatch(BC.lp(name), lanes=4, updatable=updatable, **OPTIONS)
    I, _ = _run_and_compare(name, updatable, batch, tagged)
    assert (I.lanes_concurrent, I.fallback_variants) == (4, 0), I.text
    # q_value is refused by name on such a batch, and changes nothing
    bad = [tagged[0][1], dict(q_value=np.array(BC.lp(name).hessian[2], dtype=np.float64))]
    with pytest.raises(RuntimeError, match=r"variant 1: pdlp_mi355x_update_values: the solver was not created for Hessian updates"):
        batch.run(bad)
    _run_and_compare(name, updatable, batch, tagged[:3])
    batch.close()


# ---- 5: a problem above one XCD ----------------------------------------------------------------------------------------------
def test_above_one_xcd_the_variants_run_one_after_the_other():
    name, updatable = "80bau3b", "matrix"
    tagged = [BC.matrix(name, "jitter", 71), BC.NOTHING, BC.matrix(name, "values", 72)]
    batch = solver.DeviceBatch(BC.lp(name), lanes=8, updatable=updatable, **OPTIONS)
    I, _ = _run_and_compare(name, updatable, batch, tagged)
    batch.close()
    assert I.lanes_concurrent == 1 and I.trial_launches == 0
    m = re.fullmatch(r"sequential: (\d+) work blocks need more than one XCD", I.text)
    assert m and int(m.group(1)) > 32, I.text


# ---- 6: a start and an iteration limit of its own inside a value variant ------------------------------------------------------
def test_hot_start_and_own_iteration_limit_inside_a_value_variant():
    name, updatable = "adlittle", "matrix"
    first = BC.reference(name, updatable, BC.NOTHING)[0]
    start = dict(col_value=first.col_value, row_value=first.row_value, row_dual=first.row_dual)
    tag, v = BC.matrix(name, "jitter", 81)
    tagged = [(tag, v), (tag + " hot", dict(v, start=start)), (tag + " limited", dict(v, iter_limit=80)), BC.NOTHING]
    batch = solver.DeviceBatch(BC.lp(name), lanes=3, updatable=updatable, **OPTIONS)
    I, refs = _run_and_compare(name, updatable, batch, tagged)
    batch.close()
    assert (I.lanes_concurrent, I.fallback_variants) == (3, 0), I.text
    cold, hot, limited = refs[0][0], refs[1][0], refs[2][0]
    assert limited.num_iter == 79  # (ended at its own limit: the last iteration of a run is iter_limit - 1)
    assert BC.really_differs(hot, cold)  # (the start was taken)


# ---- 7: the old entry before and after the new one, on the same batch ---------------------------------------------------------
def test_the_old_entry_before_and_after_value_variants():
    name, updatable = "adlittle", "matrix"
    plain = [BC.data(name, what, 21 + i) for i, what in enumerate(["cost", "row_bounds", "col_bounds", "all"])] + [BC.NOTHING]
    valued = [BC.matrix(name, what, 91 + i) for i, what in enumerate(["values", "all", "jitter", "decades", "signs"])]
    batch = solver.DeviceBatch(BC.lp(name), lanes=5, updatable=updatable, **OPTIONS)
    refs = _references(name, updatable, plain)
    first = batch.run([v for _, v in plain])  # (no variant has an array: pdlp_mi355x_batch_run)
    I1 = batch.info()
    _run_and_compare(name, updatable, batch, valued)
    third = batch.run([v for _, v in plain])
    I3 = batch.info()
    batch.close()
    for (tag, _), a, b, (R, _) in zip(plain, first, third, refs):
        assert BC.same_result(a.result, R) is None, (tag, "before", BC.same_result(a.result, R))
        assert BC.same_result(b.result, R) is None, (tag, "after", BC.same_result(b.result, R))
    for I in (I1, I3):
        assert (I.lanes_concurrent, I.variants, I.fallback_variants) == (5, 5, 0), I.text
        _launch_bounds(I, refs)


# ---- 8: a refusal leaves the batch as it was ---------------------------------------------------------------------------------
def test_a_refused_list_changes_nothing():
    name, updatable = "sq100", "matrix+hessian"
    P = BC.lp(name)
    good = [BC.hessian(name, "scale7"), BC.matrix(name, "values", 43), BC.NOTHING, BC.both(name, "values", "regen", 44), BC.data(name, "cost", 5)]
    q_bad = HC.doubly_wrong(P)["zero+diagonal"][0]["q_value"]
    batch = solver.DeviceBatch(P, lanes=3, updatable=updatable, **OPTIONS)
    _run_and_compare(name, updatable, batch, good[:3])
    bad = [v for _, v in good[:3]] + [dict(q_value=q_bad), good[4][1]]
    with pytest.raises(RuntimeError) as e:
        batch.run(bad)
    assert "variant 3: pdlp_mi355x_update_values: the Hessian is not positive semidefinite for this objective sense" in str(e.value)
    _run_and_compare(name, updatable, batch, good)
    bad = [good[0][1], good[1][1], dict(a_value=np.zeros(len(P.a_value))), good[3][1]]
    with pytest.raises(RuntimeError) as e:
        batch.run(bad)
    assert "variant 2: pdlp_mi355x: the LP has no rows, no columns or no matrix nonzeros" in str(e.value), str(e.value)
    _run_and_compare(name, updatable, batch, good[::-1])
    batch.close()
