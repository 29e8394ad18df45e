"""pdlp_mi355x_batch_* on the device: every R[k] of a batch must be, bit for bit, what ONE held solver gives for
update(u[k]) + run — every solution vector, count and scalar — for full lanes, refills with uneven ends, one lane, the
sequential classes (too many work blocks for one XCD, the XCD-local mode switched off), a refused batch, a QP with a
diagonal Hessian, and with solo solves of the same LP around it.  The reference is code that exists without this feature
(DeviceSolver.update + solve on a solver of its own), computed once per (instance, variant) and shared."""
import os
import re

import numpy as np
import pytest

import oraclelib as O
import qp_small_cases as QC
import update_cases as UC
from highs_amd import solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "term_iterate", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
_lps, _refs = {}, {}


def _lp(name):
    if name not in _lps:
        sub = "qp" if name.startswith("qp") else "instances"
        _lps[name] = L.HighsLp.from_npz(os.path.join(GOLD, sub, name + ".npz"))
    return _lps[name]


def _everything(lp):
    return dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)


def _variants(name, kinds, seed0=3):
    lp = _lp(name)
    return [(what + str(seed0 + i), UC.modification(lp, what, seed0 + i)) for i, what in enumerate(kinds)]


def _reference(name, tag, u, iter_limit=None, env=""):
    """Result and persistent-launch count of the solo solve of variant `tag` of instance `name`: a held solver of its own
    brought to P with u applied (every array given: whatever it held before), then run.  env: names the environment
    switches the caller has set (they are read at create), so that such a reference is one of its own."""
    key = (name, tag, iter_limit, env)
    if key not in _refs:
        lp = _lp(name)
        options = dict(OPTIONS) if iter_limit is None else dict(OPTIONS, pdlp_iteration_limit=iter_limit)
        held = solver.DeviceSolver(lp, updatable=True, **options)
        held.update(**dict(_everything(lp), **u))
        before = held.stage("persistent_launches", 1)[0]
        R = held.run(lp.num_col, lp.num_row)
        _refs[key] = (R, int(held.stage("persistent_launches", 1)[0] - before))
        held.close()
    return _refs[key]


def _assert_same_result(got, want, what):
    for k in SOLUTION:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
    for k in COUNTS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))
    for k in SCALARS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


def _run_and_compare(name, batch, tagged, limits=None):
    limits = limits or {}
    us = [dict(u, iter_limit=limits[tag]) if tag in limits else u for tag, u in tagged]
    out = batch.run(us)
    assert len(out) == len(tagged)
    for (tag, u), o in zip(tagged, out):
        _assert_same_result(o.result, _reference(name, tag, u, limits.get(tag))[0], (name, tag))
    return batch.info()


def test_full_lanes_have_the_bits_of_solo_solves_and_share_their_launches():
    name = "25fv47"  # 21 work blocks: XCD-local
    tagged = _variants(name, ["cost", "col_bounds", "row_bounds", "cost", "col_bounds", "row_bounds", "all", "cost"])
    batch = solver.DeviceBatch(_lp(name), lanes=8, **OPTIONS)
    I = _run_and_compare(name, batch, tagged)
    batch.close()
    print("batch info:", I.text, I.lanes_concurrent, I.trial_launches, I.check_launches, list(I.xcc_of_lane))
    assert I.text == "concurrent: 8 lanes, 21 workgroups each"
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (8, 8, 8, 0)
    assert sorted(I.xcc_of_lane) == list(range(8)), list(I.xcc_of_lane)  # every lane on an XCD of its own
    solo = [_reference(name, tag, u)[1] for tag, u in tagged]
    print("solo launches:", solo)
    # All eight start in the first round and nothing is refilled, so the rounds go on until the slowest variant's last
    # needed unit; a round queues at most 16 units per lane, so at most 15 launches of the last round come after it.  A solo
    # solve's own count is its needed units plus its own overshoot (>= 0), hence the bound; and far below the sum.
    assert I.trial_launches <= max(solo) + 15, (I.trial_launches, solo)
    assert 2 * I.trial_launches < sum(solo), (I.trial_launches, solo)
    assert I.check_launches == I.trial_launches + 1  # (one check per unit, and the entry's check of the first round)


@pytest.mark.parametrize("name", ["afiro", "adlittle"])
def test_refill_and_uneven_ends(name):
    lp = _lp(name)
    tagged = _variants(name, ["cost", "row_bounds", "col_bounds", "all"], seed0=21)
    first = _reference(name, "unchanged", {})[0]
    start = dict(col_value=first.col_value, row_value=first.row_value, row_dual=first.row_dual)
    tagged.insert(1, ("unchanged", {}))
    tagged.insert(3, ("hot", dict(start=start)))
    tagged.append(("limited", UC.modification(lp, "cost", 77)))
    assert len(tagged) == 7
    batch = solver.DeviceBatch(lp, lanes=3, **OPTIONS)
    I = _run_and_compare(name, batch, tagged, limits={"limited": 80})
    assert (I.lanes, I.lanes_concurrent, I.variants, I.fallback_variants) == (3, 3, 7, 0), I.text
    # the same batch again, in another order: a lane's earlier variant leaves nothing behind
    I = _run_and_compare(name, batch, tagged[::-1], limits={"limited": 80})
    assert (I.lanes_concurrent, I.fallback_variants) == (3, 0)
    batch.close()
    # (the limited variant really ended at its own limit: the last iteration of a run is iter_limit - 1)
    assert _reference(name, "limited", tagged[-1][1], 80)[0].num_iter == 79


def test_one_lane_is_a_plain_solver():
    name = "adlittle"
    tagged = _variants(name, ["cost", "row_bounds"], seed0=21)
    batch = solver.DeviceBatch(_lp(name), lanes=1, **OPTIONS)
    I = _run_and_compare(name, batch, tagged)
    batch.close()
    assert (I.lanes, I.lanes_concurrent, I.trial_launches, I.text) == (1, 1, 0, "sequential: one lane")


def test_too_many_work_blocks_for_one_xcd_run_sequentially():
    name = "80bau3b"  # more work blocks than an XCD has CUs (42 in this tree's work plan)
    tagged = _variants(name, ["cost", "col_bounds", "row_bounds"])
    batch = solver.DeviceBatch(_lp(name), lanes=4, **OPTIONS)
    I = _run_and_compare(name, batch, tagged)
    batch.close()
    assert I.lanes_concurrent == 1 and I.trial_launches == 0
    m = re.fullmatch(r"sequential: (\d+) work blocks need more than one XCD", I.text)
    assert m and int(m.group(1)) > 32, I.text


def test_xcd_local_switched_off_runs_sequentially(monkeypatch):
    name = "25fv47"
    monkeypatch.setenv("PDLP_MI355X_XCD_LOCAL", "0")  # (switches are read at create)
    tagged = _variants(name, ["cost", "col_bounds", "row_bounds"])
    batch = solver.DeviceBatch(_lp(name), lanes=4, **OPTIONS)
    out = batch.run([u for _, u in tagged])
    I = batch.info()
    batch.close()
    assert I.lanes_concurrent == 1 and I.trial_launches == 0
    assert I.text == "sequential: 21 work blocks, but the XCD-local mode is switched off"
    for (tag, u), o in zip(tagged, out):
        _assert_same_result(o.result, _reference(name, tag, u, env="XCD_LOCAL=0")[0], (name, tag))


def test_validation_is_all_or_nothing():
    name = "adlittle"
    lp = _lp(name)
    tagged = _variants(name, ["cost", "row_bounds", "col_bounds", "all"], seed0=21)
    kind = UC.row_kind(np.asarray(lp.row_lower, dtype=np.float64), np.asarray(lp.row_upper, dtype=np.float64))
    i = int(np.nonzero(kind == 0)[0][0])  # an equality row becomes a <= row
    lo = np.array(lp.row_lower, dtype=np.float64)
    lo[i] = -np.inf
    bad = [u for _, u in tagged]
    bad[2] = dict(row_lower=lo, row_upper=np.array(lp.row_upper, dtype=np.float64))
    batch = solver.DeviceBatch(lp, lanes=3, **OPTIONS)
    with pytest.raises(RuntimeError) as e:
        batch.run(bad)
    msg = str(e.value)
    assert "variant 2: pdlp_mi355x_update: row %d would change its kind from equality to <= (upper bound only)" % i in msg, msg
    I = _run_and_compare(name, batch, tagged)
    batch.close()
    assert (I.lanes_concurrent, I.variants, I.fallback_variants) == (3, 4, 0)


def test_qp_with_a_diagonal_hessian():
    name = "qp0"
    lp = _lp(name)
    tagged = _variants(name, ["cost", "col_bounds", "row_bounds", "all"], seed0=5)
    batch = solver.DeviceBatch(lp, lanes=4, **OPTIONS)
    I = _run_and_compare(name, batch, tagged)
    batch.close()
    print("qp batch info:", I.text, I.lanes_concurrent)
    # the prox step rides in the persistent loop (Solver::construct: every QP without off-diagonal entries): concurrent
    assert I.text.startswith("concurrent: 4 lanes"), I.text
    assert (I.lanes_concurrent, I.fallback_variants) == (4, 0)


def test_a_solo_solve_next_to_a_batch_keeps_its_bits():
    name = "adlittle"
    lp = _lp(name)
    before = solver.solveLpCupdlp(lp, **OPTIONS)
    tagged = _variants(name, ["cost", "row_bounds", "col_bounds"], seed0=21)
    batch = solver.DeviceBatch(lp, lanes=3, **OPTIONS)
    _run_and_compare(name, batch, tagged)
    after = solver.solveLpCupdlp(lp, **OPTIONS)
    _assert_same_result(after.result, before.result, "solo after the batch")
    _run_and_compare(name, batch, tagged)
    batch.close()
    _assert_same_result(solver.solveLpCupdlp(lp, **OPTIONS).result, before.result, "solo after the batch is gone")


# What no bit-exact test sees: how the host cuts the trials into launches.  A solve's bits do not depend on it, its host
# round trips do.  Inputs and limit are chosen so that the oracle rejects at most 8 trials in the WHOLE solve (with
# kkt_tolerance 1e-4 and a limit of 300 iterations it ends afiro at iteration 200 after 201 trials, one rejection, and
# portfolio64 at iteration 120 after 128 trials, eight rejections): then no period can outrun the 8 spare trials of its
# launch, and every scheduled check behind the start costs exactly one persistent launch.
ROUND = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=300)


@pytest.mark.parametrize("name", ["afiro", "portfolio64"])
def test_one_persistent_launch_per_period_alone_and_in_a_batch(name, monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_SLAB", "0")  # (the oracle's layout)
    lp = QC.portfolio() if name == "portfolio64" else _lp(name)
    cpu = O.oracle_solve(lp, device_reduction_order=True, device_layout="csr", **ROUND)
    print(name, "oracle: iterations", cpu.num_iter, "trials", cpu.num_trials)
    assert 0 <= cpu.num_trials - cpu.num_iter <= 8  # the precondition
    ds = solver.DeviceSolver(lp, **ROUND)
    before = ds.stage("persistent_launches", 1)[0]
    R = ds.solve().result
    launches = int(ds.stage("persistent_launches", 1)[0] - before)
    ds.close()
    assert (R.num_iter, R.num_trials) == (cpu.num_iter, cpu.num_trials)  # (the run the precondition speaks of)
    N, limit = R.num_iter, ROUND["pdlp_iteration_limit"]
    # the scheduled checks in (0, N], by the reference's rule (cupdlp_solver.c:953-962)
    U = sum(1 for it in range(1, N + 1) if it < 10 or it % 40 == 0 or it == limit - 1)
    print(name, "iterations", N, "scheduled checks", U, "persistent launches", launches)
    # (the 15: the units of a last round of 16 that lay behind the terminating one)
    assert U <= launches <= U + 15, (U, launches)
    batch = solver.DeviceBatch(lp, lanes=2, **ROUND)
    out = batch.run([{}, {}])
    I = batch.info()
    batch.close()
    print(name, "batch info:", I.text, I.lanes_concurrent, I.trial_launches, I.check_launches)
    assert (I.lanes_concurrent, I.fallback_variants) == (2, 0), I.text
    assert [o.result.num_iter for o in out] == [N, N]
    assert U <= I.trial_launches <= U + 15, (U, I.trial_launches)
    assert I.check_launches == I.trial_launches + 1
