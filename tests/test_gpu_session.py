"""pdlp_mi355x_session_solve on the device: one session takes a whole problem per call, finds on the device what differs
from the problem it holds and creates / updates / forwards — and every result must be, bit for bit, that of a FRESH
pdlp_mi355x_create + run on the same problem with the session's updatable bits (code that exists without this feature);
on LPs also that of a plain solveLpCupdlp.  The path taken and the `changed` mask are asserted at every step."""
import copy
import os

import numpy as np
import pytest

import lpgen
import update_cases as UC
import update_hessian_cases as HC
import update_matrix_cases as MC
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=20000)
SOLUTION = ("col_value", "col_dual", "row_value", "row_dual")
COUNTS = ("term_code", "num_iter", "num_trials", "num_restarts")
SCALARS = ("primal_obj", "dual_obj", "primal_feas", "dual_feas", "rel_gap", "norm_rhs", "norm_cost")
CREATE, UPDATE, UPDATE_MATRIX, UPDATE_VALUES, ONE_SHOT = (abi.SESSION_CREATE, abi.SESSION_UPDATE, abi.SESSION_UPDATE_MATRIX,
                                                          abi.SESSION_UPDATE_VALUES, abi.SESSION_ONE_SHOT)
DATA_BITS = (abi.CHANGED_COST | abi.CHANGED_COL_LOWER | abi.CHANGED_COL_UPPER | abi.CHANGED_ROW_BOUNDS | abi.CHANGED_OFFSET)

MAKERS = {
    "adlittle": lambda: L.HighsLp.from_npz(os.path.join(GOLD, "instances", "adlittle.npz")),  # persistent loop
    "random_lp": lambda: lpgen.random_lp(5),                  # ranged and free rows
    # fused slab form at the smallest shape that reaches it (the slab layout starts at 2^18 rows): 524k columns, 263k rows
    "structured_lp": lambda: lpgen.structured_lp(arcs=8192, link_rows=64),
    "random_diag_qp": lambda: lpgen.random_diag_qp(3),
    "random_sparse_qp": lambda: lpgen.random_sparse_qp(3),
}
SPARSE_SEED = {"random_sparse_qp": 3}
# a fixed, short iteration budget where a whole solve takes a second: the bits are compared all the same
SHORT = {"structured_lp": dict(pdlp_iteration_limit=300)}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name]()
    return _cache[name]


def _bits(lp):
    hess = getattr(lp, "hessian", None)
    return "matrix+hessian" if hess is not None and len(hess[2]) > 0 else "matrix"


def _fresh(lp, start=None, **options):
    """create(P, opt') + run + destroy with the session's updatable bits, on a fresh solver."""
    opts = dict(OPTIONS, updatable=_bits(lp), **options)
    handle = abi.ProblemHandle(lp, start)
    ds = solver.DeviceSolver(problem_struct=handle.struct, **opts)
    ds._keep = handle
    R = ds.run(lp.num_col, lp.num_row)
    ds.close()
    return R


def _assert_same_result(a, b, what=""):
    for k in SOLUTION:
        assert np.array_equal(getattr(a, k), getattr(b, k)), (what, k)
    for k in COUNTS:
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))
    for k in SCALARS:
        assert getattr(a, k) == getattr(b, k), (what, k, getattr(a, k), getattr(b, k))


def _solve(S, lp, start=None, **options):
    out, info = S.solve(lp, start=start, **dict(OPTIONS, **options))
    assert out.status != solver.kError, out.info.get("error")
    return out.result, info


def _other_kind(lp):
    """lp with the smallest row whose kind can be changed by one bound given another kind: (lp', row, was, now)."""
    lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
    kind = UC.row_kind(lo, up)
    eq = np.nonzero(kind == 0)[0]
    out = copy.copy(lp)
    if eq.size:  # an equality row becomes <=
        i = int(eq[0])
        lo[i] = -np.inf
        now = 1
    else:        # a <= or >= row becomes an equality
        i = int(np.nonzero((kind == 1) | (kind == 2))[0][0])
        if kind[i] == 1:
            lo[i] = up[i]
        else:
            up[i] = lo[i]
        now = 0
    out.row_lower, out.row_upper = lo, up
    return out, i, int(kind[i]), now


def _other_pattern(lp):
    """The same matrix with two entries of one column in the other order: a different pattern."""
    st = np.asarray(lp.a_start)
    j = int(np.nonzero(np.diff(st) >= 2)[0][0])
    p = int(st[j])
    out = copy.copy(lp)
    idx, val = np.array(lp.a_index), np.array(lp.a_value, dtype=np.float64)
    idx[[p, p + 1]] = idx[[p + 1, p]]
    val[[p, p + 1]] = val[[p + 1, p]]
    out.a_index, out.a_value = idx, val
    return out


# ---- the chain ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gpu_setup", ["0", "1"])
@pytest.mark.parametrize("name", list(MAKERS))
def test_chain_equals_fresh_solves(name, gpu_setup, monkeypatch):
    """P, P with every update_cases modification, new matrix values, (QPs: new Hessian values,) the first P again, P once
    more, a kind change, a pattern change — through ONE session.  (Going back to the first P from new matrix values is a
    matrix update by the ladder — a_value differs from what is held; the data-only path with nothing changed is the solve
    after it.)"""
    monkeypatch.setenv("PDLP_MI355X_GPU_SETUP", gpu_setup)
    lp = _lp(name)
    qp = _bits(lp) == "matrix+hessian"
    short = SHORT.get(name, {})
    if name == "structured_lp" and gpu_setup == "1":  # the shape must reach the form it stands for
        ds = solver.DeviceSolver(lp, **OPTIONS)
        assert ds.stage("trial_launches")[0] == 2.0, "structured_lp no longer runs the fused slab trial"
        ds.close()
    steps = [("first", lp, CREATE, None)]
    for what in UC.KINDS:
        steps.append((what, UC.apply(lp, UC.modification(lp, what, seed=len(name) + 7)), UPDATE, None))
    steps.append(("matrix values", MC.apply(lp, MC.modification(lp, "values", seed=len(name) + 13)), UPDATE_MATRIX, None))
    if qp:
        u = HC.modification(lp, "regen", seed=len(name) + 5, sparse_seed=SPARSE_SEED.get(name))
        steps.append(("hessian values", HC.apply(lp, u), UPDATE_VALUES, None))
    steps.append(("first again", lp, UPDATE_VALUES if qp else UPDATE_MATRIX, None))
    steps.append(("first once more", lp, UPDATE, 0))
    kinded, row, was, now = _other_kind(lp)
    steps.append(("kind change", kinded, CREATE, None))
    steps.append(("pattern change", _other_pattern(kinded), CREATE, None))
    S = solver.Session()
    held_bytes = None
    for what, lp_k, path, mask in steps:
        got, info = _solve(S, lp_k, **short)
        print("%s %s: %s (changed %d, diff %.3g s, set-up %.3g s)" % (name, what, info.text, info.changed, info.diff_seconds, info.setup_seconds))
        assert info.path == path, (what, info.text)
        if mask is not None:
            assert info.changed == mask, (what, info.changed)
        if what == "pattern change":  # (the two values move with their indices: they differ unless they are equal)
            assert info.changed & abi.CHANGED_PATTERN and not info.changed & ~(abi.CHANGED_PATTERN | abi.CHANGED_MATRIX_VALUES)
        if what == "kind change":
            assert (info.kind_row, info.kind_was, info.kind_now) == (row, was, now), info.text
            assert "row %d changes kind" % row in info.text
        else:
            assert info.kind_row == -1
        assert info.held_bytes > 0 and info.setup_seconds > 0.0
        if path in (UPDATE, UPDATE_MATRIX, UPDATE_VALUES):
            assert info.diff_seconds > 0.0 and info.held_bytes == held_bytes, what
        held_bytes = info.held_bytes
        _assert_same_result(got, _fresh(lp_k, **short), what)
        if not qp:  # the plain one-shot entry as well
            _assert_same_result(got, solver.solveLpCupdlp(lp_k, **dict(OPTIONS, **short)).result, what + " (plain solve)")
    S.close()


# ---- single elements, arrays that span many workgroups ---------------------------------------------------------------------
def test_single_element_changes_are_seen():
    """100k x 100k, 1M nonzeros, device set-up.  One element changes per step, each step on top of the last, at index 0,
    the last index and around a multiple of the workgroup size: the mask has exactly that array's bit and the result is
    the fresh solve's."""
    sp = solver.SyntheticProblem(100_000, 100_000, 1_000_000, 1)
    lp = sp.to_lp()
    sp.close()
    short = dict(pdlp_iteration_limit=120)
    S = solver.Session()
    got, info = _solve(S, lp, **short)
    assert info.path == CREATE
    _assert_same_result(got, _fresh(lp, **short), "first")
    cur = lp
    m, nnz = lp.num_row, len(lp.a_value)
    for array, bit, size in (("col_cost", abi.CHANGED_COST, lp.num_col), ("a_value", abi.CHANGED_MATRIX_VALUES, nnz),
                             ("a_index", abi.CHANGED_PATTERN, nnz), ("row_lower", abi.CHANGED_ROW_BOUNDS, m)):
        for pos in (0, size - 1, 256 * 37 - 1, 256 * 211 + 1):
            nxt = copy.copy(cur)
            a = np.array(getattr(cur, array))
            if array == "a_index":  # another row that the column does not have yet
                st = np.asarray(cur.a_start)
                j = int(np.searchsorted(st, pos, side="right")) - 1
                have = set(a[st[j]:st[j + 1]].tolist())
                r = (int(a[pos]) + 2) % m
                while r in have:
                    r = (r + 2) % m
                a[pos] = r
            elif array == "row_lower":  # (even rows are equalities and become ranged; odd rows stay <=: -inf -> -1e30)
                a[pos] = cur.row_upper[pos] - 0.5 if np.isfinite(a[pos]) and a[pos] > -1e20 else (-1e30 if a[pos] != -1e30 else -np.inf)
            elif array == "a_value":
                a[pos] = a[pos] * 1.5
            else:
                a[pos] = a[pos] + 1.0
            setattr(nxt, array, a)
            got, info = _solve(S, nxt, **short)
            assert info.changed == bit, (array, pos, info.changed, info.text)
            kind_changes = array == "row_lower" and pos % 2 == 0
            want = CREATE if array == "a_index" or kind_changes else UPDATE_MATRIX if array == "a_value" else UPDATE
            assert info.path == want, (array, pos, info.text)
            if kind_changes:
                assert info.kind_row == pos and (info.kind_was, info.kind_now) == (0, 3)
            _assert_same_result(got, _fresh(nxt, **short), "%s[%d]" % (array, pos))
            cur = nxt
    S.close()


# ---- run-time options ---------------------------------------------------------------------------------------------------
def test_runtime_options_reach_the_held_solver():
    lp = _lp("adlittle")
    S = solver.Session()
    got, info = _solve(S, lp, kkt_tolerance=1e-4)
    assert info.path == CREATE
    _assert_same_result(got, _fresh(lp, kkt_tolerance=1e-4))
    first_iters = got.num_iter
    got, info = _solve(S, lp, kkt_tolerance=1e-7)
    assert info.path == UPDATE and info.changed == abi.CHANGED_RUNTIME_OPTIONS, info.text
    _assert_same_result(got, _fresh(lp, kkt_tolerance=1e-7))
    assert got.num_iter > first_iters
    got, info = _solve(S, lp, kkt_tolerance=1e-7, pdlp_iteration_limit=80)
    assert info.path == UPDATE and info.changed == abi.CHANGED_RUNTIME_OPTIONS, info.text
    _assert_same_result(got, _fresh(lp, kkt_tolerance=1e-7, pdlp_iteration_limit=80))
    assert got.term_code == abi.TERM_TIMELIMIT_OR_ITERLIMIT and got.num_iter <= 80
    got, info = _solve(S, lp, pdlp_features_off=abi.FEATURE_RESTART_OFF)  # a structural one
    assert info.path == CREATE and info.changed & abi.CHANGED_STRUCTURAL_OPTIONS, info.text
    _assert_same_result(got, _fresh(lp, pdlp_features_off=abi.FEATURE_RESTART_OFF))
    S.close()


# ---- hot start ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["adlittle", "structured_lp"])
def test_hot_start_through_the_session(name):
    lp = _lp(name)
    short = dict(pdlp_iteration_limit=600) if name in SHORT else {}
    S = solver.Session()
    first, _ = _solve(S, lp, **short)
    start = dict(col_value=first.col_value.copy(), row_value=first.row_value.copy(), row_dual=first.row_dual.copy())
    lp2 = UC.apply(lp, UC.modification(lp, "cost", seed=31))
    got, info = _solve(S, lp2, start=start, **short)
    assert info.path == UPDATE and info.changed == abi.CHANGED_COST, info.text
    hot = _fresh(lp2, start=start, **short)
    _assert_same_result(got, hot, "hot")
    # the start is not sticky
    got, info = _solve(S, lp2, **short)
    assert info.path == UPDATE and info.changed == 0
    cold = _fresh(lp2, **short)
    _assert_same_result(got, cold, "cold")
    assert any(not np.array_equal(getattr(hot, k), getattr(cold, k)) for k in SOLUTION), "the start changed nothing"
    # and is honoured on the create path
    S.release()
    got, info = _solve(S, lp2, start=start, **short)
    assert info.path == CREATE
    _assert_same_result(got, hot, "hot create")
    S.close()


# ---- one-shot kinds ---------------------------------------------------------------------------------------------------------
def test_one_shot_kinds_hold_nothing(monkeypatch):
    lp = _lp("adlittle")
    S = solver.Session()
    got, info = _solve(S, lp)
    assert info.path == CREATE and info.held_bytes > 0
    out, info = S.solve(lp, solver="hipdlp", kkt_tolerance=1e-4)
    assert info.path == ONE_SHOT and info.held_bytes == 0 and "HiPDLP" in info.text
    _assert_same_result(out.result, solver.solveLpHiPdlp(lp, kkt_tolerance=1e-4).result, "hipdlp")
    got, info = _solve(S, lp)  # nothing was kept across the one-shot call
    assert info.path == CREATE
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    got, info = _solve(S, lp)
    assert info.path == ONE_SHOT and info.held_bytes == 0 and "sharded" in info.text
    _assert_same_result(got, solver.solveLpCupdlp(lp, **OPTIONS).result, "forced sharding")
    monkeypatch.delenv("PDLP_MI355X_FORCE_COMM")
    got, info = _solve(S, lp)
    assert info.path == CREATE
    S.close()


# ---- release ----------------------------------------------------------------------------------------------------------------
def test_release_and_reuse():
    lp = _lp("random_lp")
    S = solver.Session()
    first, info = _solve(S, lp)
    assert info.path == CREATE
    again, info = _solve(S, lp)
    assert info.path == UPDATE
    S.release()
    S.release()
    third, info = _solve(S, lp)
    assert info.path == CREATE and "nothing is held" in info.text
    _assert_same_result(first, again)
    _assert_same_result(first, third)
    S.close()
    S.close()


# ---- what is held ----------------------------------------------------------------------------------------------------------
def test_held_bytes_are_the_update_state_plus_the_sessions_own_buffers():
    """held_bytes minus the session's six buffers (sizes as in DESIGN §2f) is what stage("update_state") reports in [0],
    [4] and [6] for a split-ABI solver with the same bits whose staging exists (one update_matrix)."""
    lp = L.HighsLp.from_npz(os.path.join(GOLD, "instances", "afiro.npz"))
    n, m, nnz = lp.num_col, lp.num_row, len(lp.a_value)
    S = solver.Session()
    _, info = _solve(S, lp)
    assert info.path == CREATE
    own = 8 * (3 * n + 2 * m) + 8 * nnz + 4 * (n + 1 + nnz) + 8  # kept data, kept values, pattern staging, the record
    ds = solver.DeviceSolver(lp, updatable=_bits(lp), **OPTIONS)
    ds.update_matrix(np.array(lp.a_value, dtype=np.float64))
    state = ds.stage("update_state")
    assert state[0] > 0 and state[4] > 0
    assert info.held_bytes - own == state[0] + state[4] + state[6], (info.held_bytes, own, state[:8])
    ds.close()
    S.close()


# ---- the split ABI beside a live session -------------------------------------------------------------------------------------
def test_session_does_not_disturb_the_split_abi():
    lp = _lp("random_lp")
    u = UC.modification(lp, "all", seed=17)
    lp2 = UC.apply(lp, u)
    a2 = MC.modification(lp, "values", seed=19)["a_value"]
    lp3 = MC.apply(lp, dict(a_value=a2))

    def split():
        ds = solver.DeviceSolver(lp, updatable="matrix", **OPTIONS)
        ds.update(**u)
        r2 = ds.run(lp.num_col, lp.num_row)
        t2 = ds.stage("update_seconds")
        ds.update_matrix(a2, col_cost=lp.col_cost, col_lower=lp.col_lower, col_upper=lp.col_upper, row_lower=lp.row_lower,
                         row_upper=lp.row_upper, offset=lp.offset)
        r3 = ds.run(lp.num_col, lp.num_row)
        t3 = ds.stage("update_matrix_seconds")
        ds.close()
        return r2, r3, t2, t3

    alone = split()
    S = solver.Session()
    _solve(S, lp)
    _solve(S, lp2)
    beside = split()
    got, info = _solve(S, lp3)
    assert info.path == UPDATE_MATRIX
    _assert_same_result(got, _fresh(lp3))
    S.close()
    _assert_same_result(alone[0], beside[0], "update")
    _assert_same_result(alone[1], beside[1], "update_matrix")
    _assert_same_result(beside[0], _fresh(lp2), "update against fresh")
    for t in (beside[2][:3], beside[3][:5]):  # upload + validation, kernels, norms + sums (matrix: formulate, passes, refills too)
        assert all(v > 0.0 for v in t), t
    assert beside[2][6] > 0.0 and beside[3][8] > 0.0
