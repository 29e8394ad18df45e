"""The structural claim every case of tests/edge_cases.py exists for, asserted through the product's own host planners
(solver.Prepared, solver.stream_plan = planStream + planLong as the device set-up calls them, the slab layout and its task
plan), and the conditions tests/test_gpu_edges.py relies on, asserted on the oracle alone.  No GPU.

Oracle alone, device-order mode, kkt_tolerance 1e-7, capped (edge_cases.SOLVES) — iterations / trials / restarts:
  grid32 400 / 403 / 11     grid33 760 / 764 / 11     grid64 560 / 561 / 10     grid65 640 / 645 / 11
  wide10000 999 / 1053 / 11 (stops at its cap)        wide16384 520 / 549 / 12  wide16385 600 / 628 / 12
  empty_runs 80 / 82 / 7    arrow512 120 / 127 / 6    arrow513 120 / 125 / 6
  empty_runs4600 120 / 123 / 8                        arrow512n4200 200 / 211 / 8
every one holds a rejected trial (trials > iterations) and a restart."""
import numpy as np
import pytest

import edge_cases as E
import oraclelib as O
from highs_amd import solver

_cache = {}


def _prepared(key, maker, **kw):
    if key not in _cache:
        _cache[key] = solver.Prepared(maker(), **kw)
    return _cache[key]


def _plan_is_a_partition(beg, plan):
    """What every stream plan must satisfy: the blocks and the long majors together hold every major once, in order; a block
    holds at most `chunk` entries and 2048 majors and records its entry range; a long major has more than `chunk` entries."""
    chunk, covered = plan["chunk"], []
    for b0, b1, e0, e1 in plan["blocks"]:
        assert b0 < b1 <= b0 + 2048 and (e0, e1) == (beg[b0], beg[b1]) and e1 - e0 <= chunk
        covered += list(range(b0, b1))
    lens = np.diff(beg)
    assert np.array_equal(plan["long_majors"], np.nonzero(lens > chunk)[0])
    assert sorted(covered + list(plan["long_majors"])) == list(range(len(beg) - 1))
    assert plan["n_blocks"] == len(plan["blocks"]) and plan["n_long"] == len(plan["long_majors"])


def _tasks_tile_their_majors(beg, plan):
    """Segment tasks of the stream layout: per long major, in order, its segments tile its entries; returns (segments per
    long major, indices of the idle tasks, contained flags)."""
    T, W = plan["tasks"], plan["task_group"]
    assert W == 4 and T.shape == (plan["n_tasks"], 8)
    idle = [t for t in range(len(T)) if T[t, 2] < 0]
    for t in idle:
        assert T[t, 0] == T[t, 1] == 0  # (an idle task has no entries: a wave that took it as major 0 would add nothing, but store)
    segs, contained = [], []
    for c, r in enumerate(plan["long_majors"]):
        mine = [t for t in range(len(T)) if T[t, 2] == c]
        assert mine == list(range(mine[0], mine[0] + len(mine)))  # consecutive
        n_seg = len(mine)
        assert all(T[t, 3] == mine[0] and T[t, 4] == n_seg and T[t, 5] == r for t in mine)
        assert [T[t, 7] for t in mine] == list(range(n_seg))
        assert T[mine[0], 0] == beg[r] and T[mine[-1], 1] == beg[r + 1]
        assert all(T[a, 1] == T[a + 1, 0] for a in mine[:-1])
        seg_len = {int(T[t, 1] - T[t, 0]) for t in mine[:-1]}
        assert len(seg_len) <= 1 and seg_len <= {512, 1024, 2048} and 0 < T[mine[-1], 1] - T[mine[-1], 0] <= max(seg_len | {512})
        flag = {int(T[t, 6]) for t in mine}
        assert len(flag) == 1
        if flag == {1}:  # contained: all its tasks in one workgroup of W
            assert n_seg <= W and mine[0] // W == mine[-1] // W
        else:
            assert n_seg > W
        segs.append(n_seg)
        contained.append(flag.pop())
    return segs, idle, contained


# ---- majors at the limit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("chunk", [512, 2048])
def test_majors_at_limit(chunk):
    P = _prepared(("limit", chunk), lambda: E.majors_at_limit(chunk, "integer"), pdlp_features_off=1)
    assert (P.nnz < 2**18) == (chunk == 512) and np.array_equal(P.row_new_idx, np.arange(P.m))
    rows, cols = np.diff(P.csr_beg), np.diff(P.csc_beg)
    assert tuple(rows[:10]) == E.limit_rows(chunk) and rows[-1] == 0 and rows[0] == 0
    assert tuple(cols[:4]) == (0, chunk - 1, chunk + 1, chunk) and cols[-1] == 0
    assert rows[10:].max() <= (70 + 3 if chunk == 2048 else 4 + 3) and cols[4:].max() < 256
    a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
    for beg, plan in ((P.csr_beg, a), (P.csc_beg, at)):
        assert plan["chunk"] == chunk
        _plan_is_a_partition(beg, plan)
        segs, idle, contained = _tasks_tile_their_majors(beg, plan)
        assert segs == [2 if chunk == 512 else 5] and idle == [] and contained == [1 if chunk == 512 else 0]
    # chunk + 1 is long, chunk and chunk - 1 are not; its neighbours end one block and begin the next
    assert list(a["long_majors"]) == [7] and list(at["long_majors"]) == [2]
    assert 7 in a["blocks"][:, 1] and 8 in a["blocks"][:, 0] and 2 in at["blocks"][:, 1] and 3 in at["blocks"][:, 0]
    assert (a["n_blocks"], at["n_blocks"]) == (P.spmv_blocks_ax, P.spmv_blocks_aty)
    # the slab layout's limit: 257 is long, 256 and 255 are not
    assert list(P.slab_layout(0)["long_map"]) == [3, 6, 7, 8] and list(P.slab_layout(1)["long_map"]) == [1, 2, 3]
    assert list(solver.stream_plan(P, 0, 256)["long_majors"]) == [3, 6, 7, 8]


# ---- segments -----------------------------------------------------------------------------------------------------------
def test_segments():
    P = _prepared("segments", lambda: E.segments("integer"), pdlp_features_off=1)
    assert P.n >= 32769 and P.nnz == 72203 < 2**18
    assert tuple(np.diff(P.csr_beg)[1:8]) == E.SEGMENT_ROWS and np.diff(P.csc_beg).max() <= 512
    a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
    _plan_is_a_partition(P.csr_beg, a)
    _plan_is_a_partition(P.csc_beg, at)
    assert a["chunk"] == 512 and list(a["long_majors"]) == [1, 2, 3, 4, 5, 6, 7] and at["n_long"] == 0 and at["n_tasks"] == 0
    segs, idle, contained = _tasks_tile_their_majors(P.csr_beg, a)
    assert segs == [2, 3, 3, 4, 5, 64, 33]
    assert contained == [1, 1, 1, 1, 0, 0, 0]
    # 513: tasks 0-1 | two idle | 1025: 4-6 | one idle | 1025: 8-10 | one idle | 2048: 12-15, a whole workgroup | 2049: 16-20, spanning
    assert idle == [2, 3, 7, 11] and a["n_tasks"] == 21 + 64 + 33
    T = a["tasks"]
    assert {int(t[1] - t[0]) for t in T if t[2] == 5} == {512}  # 32768 entries: 64 segments of 512
    assert sorted({int(t[1] - t[0]) for t in T if t[2] == 6}) == [1, 1024]  # 32769: 32 of 1024 and one entry
    # the slab layout cuts the same majors into the same segments (contained there means one segment)
    S = P.task_plan(0)
    assert S["n_long"] == 7 and [int(S["tasks"][S["tasks"][:, 2] == c][0, 4]) for c in range(7)] == segs
    assert a["long_group"] == 1 == solver.stream_plan(P, 0, 256)["long_group"]


# ---- more long majors than contribution slots ---------------------------------------------------------------------------
@pytest.mark.parametrize("k,group,slots", [(2048, 1, 2048), (2049, 2, 1025)])
def test_many_long(k, group, slots):
    """Slab layout only: a stream-layout operand reaches the cap with 2049 majors beyond its chunk, and the chunk is 2048 from
    2^18 nonzeros on (2049 rows of 513 entries are 1.05M nonzeros, hence chunk 2048, hence 2049 rows of 2049: 4.2M) — no small
    case exists."""
    P = _prepared(("long", k), lambda: E.many_long(k, "integer"), pdlp_features_off=1)
    rows, cols = np.diff(P.csr_beg), np.diff(P.csc_beg)
    assert (rows == 257).sum() == k and (rows > 256).sum() == k and cols.max() <= 256 and P.nnz < 0.54e6
    a, at = solver.stream_plan(P, 0, 256), solver.stream_plan(P, 1, 256)
    assert (a["n_long"], a["long_group"], a["long_slots"]) == (k, group, slots)
    assert (at["n_long"], at["long_group"]) == (0, 1)
    assert P.slab_layout(0)["long_map"].size == k and P.task_plan(0)["n_long"] == k
    assert list(a["long_majors"]) == list(range(k))


# ---- runs of empty majors -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("long_row", [2500, 4600])
def test_empty_runs(long_row):
    """The rows the case prescribes (long_row = 2500) give A two blocks capped at 2048 majors that hold 3 and 1 entries, and A' a
    capped block without any entry; with the 512-entry row at 4600, A has a capped block without entries too."""
    P = _prepared(("empty", long_row), lambda: E.empty_runs("integer", long_row=long_row), pdlp_features_off=1)
    rows = np.diff(P.csr_beg)
    assert P.m == 6000 and (rows[0], rows[long_row], rows[long_row + 1], rows[-1]) == (3, 512, 1, 2) and rows.sum() == 518 == P.nnz
    a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
    _plan_is_a_partition(P.csr_beg, a)
    _plan_is_a_partition(P.csc_beg, at)
    if long_row == 2500:
        assert a["blocks"].tolist() == [[0, 2048, 0, 3], [2048, 2501, 3, 515], [2501, 4549, 515, 516], [4549, 6000, 516, 518]]
    else:  # block 1: 2048 majors, first entry == end entry
        assert a["blocks"].tolist() == [[0, 2048, 0, 3], [2048, 4096, 3, 3], [4096, 4601, 3, 515], [4601, 6000, 515, 518]]
    assert at["blocks"].tolist() == [[0, 508, 0, 512], [508, 2556, 512, 516], [2556, 4604, 516, 516], [4604, 6000, 516, 518]]
    assert (np.diff(P.csc_beg)[512:5998] == 0).all()  # the run of empty columns
    assert (P.spmv_blocks_ax, P.spmv_blocks_aty) == (4, 4) and a["n_long"] == at["n_long"] == 0
    assert a["small_grid"] == 24  # ceil(6000 / 256): twenty workgroups of the persistent loop own no block at all


# ---- the persistent grid ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("g", [32, 33, 64, 65])
def test_grid(g):
    P = _prepared(("grid", g), lambda: E.grid(g))
    assert (P.m, P.n) == E.GRID_SHAPES[g] and P.nnz == P.m * P.n
    a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
    _plan_is_a_partition(P.csr_beg, a)
    _plan_is_a_partition(P.csc_beg, at)
    assert (P.spmv_blocks_ax, P.spmv_blocks_aty, a["n_blocks"], at["n_blocks"]) == (g, g, g, g)
    assert a["n_long"] == at["n_long"] == 0 and a["chunk"] == at["chunk"] == 512
    assert a["small_grid"] == g


@pytest.mark.parametrize("n,blocks_aty,gv,grid", [(10000, 8, 40, 40), (16384, 11, 64, 64), (16385, 11, 65, 64)])
def test_wide(n, blocks_aty, gv, grid):
    P = _prepared(("wide", n), lambda: E.wide(n))
    rows, cols = np.diff(P.csr_beg), np.diff(P.csc_beg)
    assert P.n == n and list(rows) == [500] * 4 and (cols[:2000] == 1).all() and (cols[2000:] == 0).all()
    assert (P.cost != 0).all() and np.isfinite(P.lower).all() and np.isfinite(P.upper).all()
    a, at = solver.stream_plan(P, 0), solver.stream_plan(P, 1)
    _plan_is_a_partition(P.csr_beg, a)
    _plan_is_a_partition(P.csc_beg, at)
    assert (P.spmv_blocks_ax, P.spmv_blocks_aty) == (4, blocks_aty) == (a["n_blocks"], at["n_blocks"])
    assert -(-n // 256) == gv and a["small_grid"] == grid
    assert max(0, n - grid * 256) == (1 if n == 16385 else 0)  # columns left to the strided pass of the column step


# ---- the small QP -------------------------------------------------------------------------------------------------------
def _n_operand(hess, n):
    return dict(n=n, m=n, nnz=hess["nnz_off"], spmv_blocks_ax=0, spmv_blocks_aty=0,
                **{o + s: hess["q" + s] for o in ("csr", "csc") for s in ("_beg", "_idx", "_val")})


@pytest.mark.parametrize("k", [512, 513])
def test_arrow_qp(k):
    form, hess = solver.host_prepare_qp(E.arrow_qp(k))
    lens = np.diff(hess["q_beg"])
    assert lens[0] == k and (lens[1:k + 1] == 1).all() and (lens[k + 1:] == 0).all() and lens.size == 700
    pn = solver.stream_plan(_n_operand(hess, 700), 0)
    _plan_is_a_partition(hess["q_beg"], pn)
    assert pn["chunk"] == 512
    if k == 512:  # no long major: N qualifies; the empty majors join the block of the single entries
        assert pn["n_long"] == 0 and pn["blocks"].tolist() == [[0, 1, 0, 512], [1, 700, 512, 1024]]
    else:
        assert list(pn["long_majors"]) == [0] and pn["n_tasks"] == 2
    # A: two long rows as segment tasks and one block (the short third row); A': 3 blocks; the grid: 3 workgroups
    pa, pat = solver.stream_plan(form, 0, 0, pn["n_blocks"]), solver.stream_plan(form, 1)
    assert (pa["n_blocks"], pa["n_long"], pa["n_tasks"], pat["n_blocks"], pat["n_long"]) == (1, 2, 4, 3, 0)
    assert pa["small_grid"] == 3 > pn["n_blocks"]  # (k = 512: workgroup 2 has no block of N)


def test_arrow_qp_on_4200_columns_has_blocks_of_n_without_entries():
    form, hess = solver.host_prepare_qp(E.arrow_qp(512, n=4200))
    lens = np.diff(hess["q_beg"])
    assert lens[0] == 512 and (lens[1:513] == 1).all() and (lens[513:] == 0).all() and lens.size == 4200
    pn = solver.stream_plan(_n_operand(hess, 4200), 0)
    _plan_is_a_partition(hess["q_beg"], pn)
    # the full block | 2048 majors, capped | 2048 majors without an entry | the rest, without an entry
    assert pn["n_long"] == 0 and pn["blocks"].tolist() == [[0, 1, 0, 512], [1, 2049, 512, 1024], [2049, 4097, 1024, 1024], [4097, 4200, 1024, 1024]]
    pa, pat = solver.stream_plan(form, 0, 0, pn["n_blocks"]), solver.stream_plan(form, 1)
    # A: two rows of 4200 entries, 9 spanning segment tasks each, and the short row's block; A': 17 blocks; ceil(4200 / 256) = 17
    assert (pa["n_blocks"], pa["n_long"], pa["n_tasks"], pat["n_blocks"], pat["n_long"]) == (1, 2, 18, 17, 0)
    assert pa["small_grid"] == 17


def test_exact_major_sums_against_rational_arithmetic():
    """The order-free reference of the GPU tests, itself against fractions.Fraction on a few majors of each kind."""
    from fractions import Fraction
    P = _prepared(("limit-real", 512), lambda: E.majors_at_limit(512))
    x = np.random.default_rng(1).standard_normal(P.n)
    exact, scale, lens = E.exact_major_sums(P.csr_beg, P.csr_idx, P.csr_val, x)
    for r in (0, 1, 2, 3, 6, 7, 8, 9, 200, P.m - 1):
        sl = slice(P.csr_beg[r], P.csr_beg[r + 1])
        terms = [Fraction(float(a)) * Fraction(float(b)) for a, b in zip(P.csr_val[sl], x[P.csr_idx[sl]])]
        assert exact[r] == float(sum(terms, Fraction(0))) and lens[r] == len(terms)  # (float(Fraction) rounds to nearest)
        rounded = [Fraction(abs(float(a) * float(b))) for a, b in zip(P.csr_val[sl], x[P.csr_idx[sl]])]
        assert scale[r] == float(sum(rounded, Fraction(0)))  # the sum of the rounded |products|, rounded once


# ---- what the GPU tests rely on, on the oracle alone --------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(E.SOLVES))
def test_oracle_alone_rejects_a_trial_and_restarts_inside_the_cap(name):
    maker, cap = E.SOLVES[name]
    R = O.oracle_solve(maker(), device_reduction_order=True, device_layout="csr", kkt_tolerance=1e-7, pdlp_iteration_limit=cap)
    print(name, "iterations", R.num_iter, "trials", R.num_trials, "restarts", R.num_restarts, "term", R.term_code)
    assert R.num_trials > R.num_iter and R.num_restarts >= 1
    assert R.num_iter > 41  # (the switch tests compare the state after 40 and 41 iterations)
