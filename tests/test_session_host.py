"""The session's decision without a GPU: pdlp_mi355x_host_classify is the host twin of what pdlp_mi355x_session_solve
finds on the device — the same ladder function (one-shot / create / update values / update matrix / update), the same
`changed` mask, the same reason words — plus the fixed points of the ABI and the session entries that need no device."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import lpgen
import update_cases as UC
import update_hessian_cases as HC
import update_matrix_cases as MC
from highs_amd import abi, solver
from highs_amd import lp as L

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NONE, CREATE, UPDATE, UPDATE_MATRIX, UPDATE_VALUES, ONE_SHOT = range(6)
BIT = {"col_cost": abi.CHANGED_COST, "col_lower": abi.CHANGED_COL_LOWER, "col_upper": abi.CHANGED_COL_UPPER,
       "row_lower": abi.CHANGED_ROW_BOUNDS, "row_upper": abi.CHANGED_ROW_BOUNDS, "offset": abi.CHANGED_OFFSET}
MAKERS = {
    "afiro": lambda: L.HighsLp.from_npz(os.path.join(GOLD, "instances", "afiro.npz")),
    "adlittle": lambda: L.HighsLp.from_npz(os.path.join(GOLD, "instances", "adlittle.npz")),
    "random_lp": lambda: lpgen.random_lp(5),
    "random_sparse_qp": lambda: lpgen.random_sparse_qp(3),
}
_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name]()
    return _cache[name]


@pytest.fixture(params=list(MAKERS))
def lp(request):
    return _lp(request.param)


def _with(lp, **arrays):
    out = copy.copy(lp)
    for k, v in arrays.items():
        setattr(out, k, v)
    return out


# ---- the ladder ----------------------------------------------------------------------------------------------------------
def test_nothing_held_is_a_create(lp):
    I = solver.host_classify(None, lp)
    assert (I.path, I.changed, I.kind_row) == (CREATE, 0, -1) and "nothing is held" in I.text


def test_nothing_changed_is_an_update_with_an_empty_mask(lp):
    I = solver.host_classify(lp, copy.copy(lp))
    assert (I.path, I.changed, I.kind_row, I.kind_was, I.kind_now) == (UPDATE, 0, -1, -1, -1), I.text
    assert "nothing differs" in I.text
    assert (I.diff_seconds, I.upload_seconds, I.apply_seconds, I.setup_seconds, I.held_bytes) == (0.0, 0.0, 0.0, 0.0, 0)


@pytest.mark.parametrize("what", UC.KINDS)
def test_data_changes_are_updates_with_exactly_their_bits(lp, what):
    u = UC.modification(lp, what, seed=11)
    want = 0
    for k, v in u.items():
        same = v == lp.offset if k == "offset" else np.array_equal(np.asarray(v).view(np.uint64), np.asarray(getattr(lp, k), dtype=np.float64).view(np.uint64))
        want |= 0 if same else BIT[k]
    assert want, "the modification changes nothing"
    I = solver.host_classify(lp, UC.apply(lp, u))
    assert (I.path, I.changed) == (UPDATE, want), I.text
    assert I.text.startswith("update: ") and "differ" in I.text
    for bit, word in ((abi.CHANGED_COST, "costs"), (abi.CHANGED_ROW_BOUNDS, "row bounds"), (abi.CHANGED_COL_LOWER, "column lower bounds"),
                      (abi.CHANGED_COL_UPPER, "column upper bounds"), (abi.CHANGED_OFFSET, "offset")):
        assert (word in I.text) == bool(want & bit), (word, I.text)


def test_new_matrix_values_are_a_matrix_update(lp):
    I = solver.host_classify(lp, _with(lp, a_value=np.asarray(lp.a_value) * 2.0))
    assert (I.path, I.changed) == (UPDATE_MATRIX, abi.CHANGED_MATRIX_VALUES) and "matrix values differ" in I.text
    both = UC.apply(_with(lp, a_value=np.asarray(lp.a_value) * 2.0), UC.modification(lp, "cost", seed=3))
    I = solver.host_classify(lp, both)
    assert (I.path, I.changed) == (UPDATE_MATRIX, abi.CHANGED_MATRIX_VALUES | abi.CHANGED_COST) and "costs" in I.text


def test_new_hessian_values_are_a_values_update():
    lp = _lp("random_sparse_qp")
    u = HC.modification(lp, "scale7", seed=5, sparse_seed=3)
    I = solver.host_classify(lp, HC.apply(lp, u))
    assert (I.path, I.changed) == (UPDATE_VALUES, abi.CHANGED_HESSIAN_VALUES) and "Hessian values differ" in I.text
    with_matrix = _with(HC.apply(lp, u), a_value=np.asarray(lp.a_value) * 0.5)
    I = solver.host_classify(lp, with_matrix)
    assert (I.path, I.changed) == (UPDATE_VALUES, abi.CHANGED_HESSIAN_VALUES | abi.CHANGED_MATRIX_VALUES), I.text
    # the Hessian's pattern, and a Hessian that appears or disappears
    st, idx, val = lp.hessian
    idx2 = np.array(idx)
    j = int(np.nonzero(np.diff(st) >= 2)[0][0])
    idx2[[st[j], st[j] + 1]] = idx2[[st[j] + 1, st[j]]]
    moved = copy.copy(lp)
    moved.hessian = (st, idx2, val)
    I = solver.host_classify(lp, moved)
    assert I.path == CREATE and I.changed & abi.CHANGED_HESSIAN_PATTERN and "Hessian pattern" in I.text
    plain = copy.copy(lp)
    plain.hessian = None
    for a, b in ((lp, plain), (plain, lp)):
        I = solver.host_classify(a, b)
        assert (I.path, I.changed) == (CREATE, abi.CHANGED_SHAPE), I.text


def test_a_permuted_column_is_a_new_pattern(lp):
    st = np.asarray(lp.a_start)
    j = int(np.nonzero(np.diff(st) >= 2)[0][0])
    p = int(st[j])
    idx = np.array(lp.a_index)
    idx[[p, p + 1]] = idx[[p + 1, p]]
    I = solver.host_classify(lp, _with(lp, a_index=idx))
    assert (I.path, I.changed) == (CREATE, abi.CHANGED_PATTERN) and "matrix pattern differs" in I.text


def test_one_more_column_and_a_flipped_sense_are_creates(lp):
    wider = copy.copy(lp)
    wider.num_col = lp.num_col + 1
    wider.a_start = np.append(np.asarray(lp.a_start), np.asarray(lp.a_start)[-1]).astype(np.int32)
    for k in ("col_cost", "col_lower", "col_upper"):
        setattr(wider, k, np.append(np.asarray(getattr(lp, k), dtype=np.float64), 0.0))
    if getattr(lp, "hessian", None) is not None:
        wider.hessian = lp.hessian
    I = solver.host_classify(lp, wider)
    assert (I.path, I.changed) == (CREATE, abi.CHANGED_SHAPE) and "sizes" in I.text
    I = solver.host_classify(lp, _with(lp, sense=-lp.sense))
    assert (I.path, I.changed) == (CREATE, abi.CHANGED_SHAPE) and "sense" in I.text


def test_a_row_that_changes_kind_is_a_create_that_names_it(lp):
    lo, up = np.array(lp.row_lower, dtype=np.float64), np.array(lp.row_upper, dtype=np.float64)
    kind = UC.row_kind(lo, up)
    eq = np.nonzero(kind == 0)[0]
    assert eq.size >= 2
    for i in (int(eq[-1]), int(eq[0])):  # two rows change: the smallest is reported
        lo[i] = -np.inf
    I = solver.host_classify(lp, _with(lp, row_lower=lo))
    assert (I.path, I.changed) == (CREATE, abi.CHANGED_ROW_BOUNDS)
    assert (I.kind_row, I.kind_was, I.kind_now) == (int(eq[0]), 0, 1)
    assert I.text == "create: row %d changes kind: equality -> <=" % int(eq[0])


def test_options(lp):
    I = solver.host_classify(lp, lp, held_options=dict(kkt_tolerance=1e-4), kkt_tolerance=1e-4, gap_tol=1e-6)
    assert (I.path, I.changed) == (UPDATE, abi.CHANGED_RUNTIME_OPTIONS) and "run-time options" in I.text
    I = solver.host_classify(lp, lp, pdlp_iteration_limit=80, log_level=1)
    assert (I.path, I.changed) == (UPDATE, abi.CHANGED_RUNTIME_OPTIONS)
    I = solver.host_classify(lp, lp, pdlp_features_off=abi.FEATURE_RESTART_OFF)
    assert I.path == CREATE and I.changed == abi.CHANGED_STRUCTURAL_OPTIONS and "structural option" in I.text
    for structural in (dict(check_interval=20), dict(restart_method=0), dict(updatable="matrix"), dict(device=1)):
        assert solver.host_classify(lp, lp, **structural).path == CREATE, structural
    # a structural option and a run-time one: create, both bits, and the arrays are not even looked at
    I = solver.host_classify(lp, _with(lp, a_value=np.asarray(lp.a_value) * 2.0), pdlp_features_off=1, kkt_tolerance=1e-3)
    assert I.path == CREATE and I.changed == abi.CHANGED_STRUCTURAL_OPTIONS | abi.CHANGED_RUNTIME_OPTIONS


def test_one_shot_kinds(lp, monkeypatch):
    I = solver.host_classify(lp, lp, solver="hipdlp")
    assert (I.path, I.changed) == (ONE_SHOT, 0) and "HiPDLP" in I.text
    I = solver.host_classify(lp, lp, num_devices=2)
    assert (I.path, I.changed) == (ONE_SHOT, 0) and "sharded" in I.text
    assert solver.host_classify(None, lp, num_devices=2).path == ONE_SHOT
    monkeypatch.setenv("PDLP_MI355X_DEVICES", "4")
    assert solver.host_classify(lp, lp).path == ONE_SHOT
    assert solver.host_classify(lp, lp, num_devices=1).path == UPDATE  # the field wins over the environment
    monkeypatch.delenv("PDLP_MI355X_DEVICES")
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    I = solver.host_classify(lp, lp)
    assert I.path == ONE_SHOT and "forced" in I.text


# ---- the comparison is on bit patterns, element by element ------------------------------------------------------------------
@pytest.mark.parametrize("array,bit,path", [("col_cost", abi.CHANGED_COST, UPDATE), ("a_value", abi.CHANGED_MATRIX_VALUES, UPDATE_MATRIX),
                                            ("row_upper", abi.CHANGED_ROW_BOUNDS, UPDATE)])
def test_one_element(array, bit, path):
    lp = _lp("random_lp")
    a = np.asarray(getattr(lp, array), dtype=np.float64)
    kind = UC.row_kind(np.asarray(lp.row_lower, dtype=np.float64), np.asarray(lp.row_upper, dtype=np.float64))
    for pos in (0, a.size - 1, a.size // 2):
        b = a.copy()
        if array == "row_upper":  # keep the row's kind: an equality would need both bounds, an infinite bound another infinite
            if kind[pos] == 0:
                lo = np.array(lp.row_lower, dtype=np.float64)
                lo[pos] += 0.25
                b[pos] += 0.25
                I = solver.host_classify(lp, _with(lp, row_lower=lo, row_upper=b))
                assert (I.path, I.changed, I.kind_row) == (UPDATE, bit, -1), (pos, I.text)
                continue
            b[pos] = b[pos] + 0.25 if b[pos] < 1e20 else (1e30 if b[pos] != 1e30 else np.inf)
        else:
            b[pos] = b[pos] * 1.5 + 0.125
        I = solver.host_classify(lp, _with(lp, **{array: b}))
        assert (I.path, I.changed, I.kind_row) == (path, bit, -1), (array, pos, I.text)


def test_negative_zero_differs_and_an_equal_copy_does_not():
    lp = _lp("random_lp")
    c = np.array(lp.col_cost, dtype=np.float64)
    c[3] = 0.0
    held = _with(lp, col_cost=c)
    d = c.copy()
    assert d.ctypes.data != c.ctypes.data
    I = solver.host_classify(held, _with(lp, col_cost=d))
    assert (I.path, I.changed) == (UPDATE, 0)
    d[3] = -0.0
    assert d[3] == c[3]
    I = solver.host_classify(held, _with(lp, col_cost=d))
    assert (I.path, I.changed) == (UPDATE, abi.CHANGED_COST)
    # NaN payloads compare as bits: the same NaN is unchanged, another payload is a change
    nan_a = np.array([0x7ff8000000000001], dtype=np.uint64).view(np.float64)[0]
    nan_b = np.array([0x7ff8000000000002], dtype=np.uint64).view(np.float64)[0]
    ca, cb = c.copy(), c.copy()
    ca[1], cb[1] = nan_a, nan_b
    assert solver.host_classify(_with(lp, col_cost=ca), _with(lp, col_cost=ca.copy())).changed == 0
    assert solver.host_classify(_with(lp, col_cost=ca), _with(lp, col_cost=cb)).changed == abi.CHANGED_COST


# ---- the ABI's fixed points ----------------------------------------------------------------------------------------------------
def test_the_abi_is_extended_not_changed():
    lib = solver.lib()
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(1) == 104 == C.sizeof(abi.PdlpParams)
    assert lib.pdlp_mi355x_sizeof(9) == -1
    assert lib.pdlp_mi355x_session_info_size() == C.sizeof(abi.PdlpSessionInfo) == 224
    for name in ("pdlp_mi355x_session_create", "pdlp_mi355x_session_solve", "pdlp_mi355x_session_info", "pdlp_mi355x_session_release",
                 "pdlp_mi355x_session_destroy", "pdlp_mi355x_session_info_size", "pdlp_mi355x_host_classify"):
        assert name in solver.EXPORTS and hasattr(lib, name)


def test_an_empty_session_needs_no_gpu():
    S = solver.Session()
    I = S.info
    assert (I.path, I.changed, I.kind_row, I.held_bytes) == (NONE, 0, -1, 0) and "nothing solved" in I.text
    S.release()
    S.release()
    assert S.info.path == NONE
    S.close()
    S.close()
    lib = solver.lib()
    assert lib.pdlp_mi355x_session_create(None) != 0 and b"null" in lib.pdlp_mi355x_last_error()
    assert lib.pdlp_mi355x_session_info(None, None) != 0
    lib.pdlp_mi355x_session_release(None)
    lib.pdlp_mi355x_session_destroy(None)
