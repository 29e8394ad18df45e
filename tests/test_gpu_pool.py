"""pdlp_mi355x_solve_many on the device: every R[k] of a pool must be, bit for bit, what a solver of its own gives for
create + run — every solution vector, count and scalar — for eight different instances on eight lanes, lanes that differ in
barriers per trial, refills with uneven ends around a problem that does not qualify, one lane, the same instance eight
times, a QP, an infeasible LP and a hot start, and with solo solves and a batch around it.  The reference is code that
exists without this feature (DeviceSolver(lp, **options).run), computed once per instance and shared."""
import os
import re

import numpy as np
import pytest

import update_cases as UC
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=2000)
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "term_iterate", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
_lps, _solos = {}, {}


def _lp(name):
    if name not in _lps:
        sub = "qp" if name.startswith("qp") else "instances"
        _lps[name] = L.HighsLp.from_npz(os.path.join(GOLD, sub, name + ".npz"))
    return _lps[name]


def _solo(name, start=None):
    """(result, persistent launches, barriers per trial) of the solo solve of instance `name`: a solver of its own, run once.
    start: the tag of a hot start — the solo solution of the same instance."""
    key = (name, start)
    if key not in _solos:
        lp = _lp(name)
        handle = abi.ProblemHandle(lp, _start_of(name) if start else None)
        S = solver.DeviceSolver(problem_struct=handle.struct, **OPTIONS)
        barriers = int(S.stage("trial_barriers", 1)[0])
        R = S.run(lp.num_col, lp.num_row)
        _solos[key] = (R, int(S.stage("persistent_launches", 1)[0]), barriers)
        S.close()
    return _solos[key]


def _start_of(name):
    first = _solo(name)[0]
    return dict(col_value=first.col_value, row_value=first.row_value, row_dual=first.row_dual)


def _assert_same_result(got, want, what):
    for k in SOLUTION:
        assert np.array_equal(getattr(got, k), getattr(want, k)), (what, k)
    for k in COUNTS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))
    for k in SCALARS:
        assert getattr(got, k) == getattr(want, k), (what, k, getattr(got, k), getattr(want, k))


def _pool(names, lanes, hot=()):
    """solve_many on the instances `names` (those in `hot` from their solo solution) -> (paths, info); every result is
    compared with its solo solve."""
    refs = [_solo(n, "hot" if n in hot else None)[0] for n in names]  # (before the call: nothing of it can leak into them)
    starts = [_start_of(n) if n in hot else None for n in names]
    out, I = solver.solve_many([_lp(n) for n in names], lanes=lanes, starts=starts, **OPTIONS)
    assert len(out) == len(names)
    for n, o, ref in zip(names, out, refs):
        _assert_same_result(o.result, ref, n)
    print("pool info:", I.text, "concurrent", I.lanes_concurrent, "shared/alone/fallback", I.shared_problems, I.alone_problems,
          I.fallback_problems, "launches", I.trial_launches, I.check_launches, I.mixed_launches, list(I.xcc_of_lane))
    assert (I.problems, I.lanes) == (len(names), lanes)
    return [o.info["pool_path"] for o in out], I


def test_eight_different_instances_have_the_bits_of_solo_solves_and_share_their_launches():
    names = ["afiro", "adlittle", "25fv47", "e226", "sctest", "stair", "israel", "scrs8"]  # 1 to 21 work blocks: all XCD-local
    paths, I = _pool(names, 8)
    assert paths == [abi.POOL_SHARED] * 8, (paths, I.text)
    assert (I.lanes_concurrent, I.shared_problems, I.alone_problems, I.fallback_problems) == (8, 8, 0, 0)
    assert I.text == "concurrent: 8 lanes"
    assert sorted(I.xcc_of_lane) == list(range(8)), list(I.xcc_of_lane)  # every lane on an XCD of its own
    solo = [_solo(n)[1] for n in names]
    print("solo launches:", solo)
    # K <= lanes: all eight start in the first round and nothing is refilled, so the rounds go on until the slowest problem's
    # last needed unit; a round queues at most 16 units per lane, so at most 15 launches of the last round come after it.  A
    # solo solve's own count is its needed units plus its own overshoot (>= 0), hence the bound; and far below the sum.
    assert I.trial_launches <= max(solo) + 15, (I.trial_launches, solo)
    assert 2 * I.trial_launches < sum(solo), (I.trial_launches, solo)
    assert I.check_launches == I.trial_launches + 1  # (one check per unit, and the entry's check of the first round)


def test_lanes_of_two_and_three_barriers_per_trial_share_launches():
    names = ["standmps", "afiro", "adlittle", "standata", "e226", "sctest"]
    barriers = {n: _solo(n)[2] for n in names}
    print("barriers per trial:", barriers)
    assert set(barriers.values()) == {2, 3}, barriers  # at least one instance of each kind
    assert barriers["standmps"] == 3  # (its long rows keep the P phase)
    paths, I = _pool(names, 8)
    assert paths == [abi.POOL_SHARED] * len(names), (paths, I.text)
    assert I.mixed_launches > 0 and I.mixed_launches <= I.trial_launches
    assert (I.lanes_concurrent, I.fallback_problems) == (len(names), 0)


def test_refill_uneven_ends_and_a_problem_that_does_not_qualify():
    names = ["afiro", "adlittle", "sctest", "e226", "80bau3b", "stair", "standmps", "israel", "25fv47"]
    for order in (names, names[::-1]):
        paths, I = _pool(order, 3)
        k = order.index("80bau3b")
        assert paths[k] == abi.POOL_ALONE and paths[:k] + paths[k + 1:] == [abi.POOL_SHARED] * 8, (paths, I.text)
        m = re.fullmatch(r"(\d+) work blocks need more than one XCD", I.text)
        assert m and int(m.group(1)) > 32, I.text
        assert (I.lanes_concurrent, I.shared_problems, I.alone_problems, I.fallback_problems) == (3, 8, 1, 0)


def test_one_lane_is_a_loop_of_ordinary_solves():
    paths, I = _pool(["adlittle", "afiro", "standmps"], 1)
    assert paths == [abi.POOL_ALONE] * 3
    assert (I.lanes_concurrent, I.trial_launches, I.check_launches, I.text) == (1, 0, 0, "sequential: one lane")


def test_the_same_instance_eight_times():
    lp = _lp("adlittle")
    out, I = solver.solve_many([lp] * 8, lanes=8, **OPTIONS)
    for o in out:
        _assert_same_result(o.result, _solo("adlittle")[0], "adlittle")
        _assert_same_result(o.result, out[0].result, "adlittle among themselves")
    assert (I.lanes_concurrent, I.shared_problems, I.mixed_launches) == (8, 8, 0)


def test_a_qp_an_infeasible_lp_and_a_hot_start_beside_lps():
    names = ["afiro", "qp0", "galenet", "e226", "adlittle", "woodinfe"]
    paths, I = _pool(names, 4, hot=("adlittle",))
    print("paths:", dict(zip(names, paths)))
    # (the solo term code is the pool's: _pool compares it like every count; this pins that it is the infeasible one)
    assert _solo("galenet")[0].term_code in (abi.TERM_INFEASIBLE, abi.TERM_INFEASIBLE_OR_UNBOUNDED)
    hot, cold = _solo("adlittle", "hot")[0], _solo("adlittle")[0]
    assert hot.num_iter < cold.num_iter  # the start was honoured: the solo solve from it is another, shorter solve
    assert I.fallback_problems == 0 and I.lanes_concurrent >= 2


def test_solo_solves_and_a_batch_around_a_pool_keep_their_bits():
    name = "25fv47"
    lp = _lp(name)
    kinds = ["cost", "col_bounds", "row_bounds", "cost", "col_bounds", "row_bounds", "all", "cost"]  # test_gpu_batch.py's test 1
    us = [UC.modification(lp, what, 3 + i) for i, what in enumerate(kinds)]

    def batch():
        b = solver.DeviceBatch(lp, lanes=8, **OPTIONS)
        out = b.run(us)
        I = b.info()
        b.close()
        return out, I

    solo_before = solver.solveLpCupdlp(_lp("adlittle"), **OPTIONS)
    batch_before, I0 = batch()
    _pool(["standmps", "afiro", "25fv47", "standata", "e226"], 8)  # (a pool whose launches mix the two kinds)
    batch_after, I1 = batch()
    solo_after = solver.solveLpCupdlp(_lp("adlittle"), **OPTIONS)
    _assert_same_result(solo_after.result, solo_before.result, "solo around the pool")
    _assert_same_result(solo_after.result, _solo("adlittle")[0], "solo against a held solver")
    for k, (a, b) in enumerate(zip(batch_before, batch_after)):
        _assert_same_result(b.result, a.result, ("batch variant", k))
    # the batch launches what it launched before the pools (uniform lanes kernels only): its counts obey test 1's bounds of
    # test_gpu_batch.py, with the solo launch counts of its own variants
    full = dict(col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                row_upper=lp.row_upper, offset=lp.offset)
    solo = []
    held = solver.DeviceSolver(lp, updatable=True, **OPTIONS)
    for k, u in enumerate(us):
        held.update(**dict(full, **u))
        before = held.stage("persistent_launches", 1)[0]
        _assert_same_result(batch_after[k].result, held.run(lp.num_col, lp.num_row), ("batch variant against update + run", k))
        solo.append(int(held.stage("persistent_launches", 1)[0] - before))
    held.close()
    for I in (I0, I1):
        assert I.text == "concurrent: 8 lanes, 21 workgroups each"
        assert (I.lanes_concurrent, I.fallback_variants) == (8, 0)
        assert I.trial_launches <= max(solo) + 15 and 2 * I.trial_launches < sum(solo), (I.trial_launches, solo)
        assert I.check_launches == I.trial_launches + 1
