"""pdlp_mi355x_update_matrix without a GPU, through its host twin pdlp_mi355x_host_prepare_updated_matrix: prepare P,
keep the pattern, the passes and the unscaled data, apply new matrix values (and data) as the device does — the result
must be, bit for bit and in EVERY field, what pdlp_mi355x_host_prepare gives on the modified problem P' built in Python.
host_prepare is pinned on the oracle by tests/test_host.py, so this ties the matrix update to the reference.  Also: a
matrix update followed by a data update replays the NEW factors, every refusal that needs no solver handle, and the ABI
numbers this change must not move."""
import copy
import ctypes as C
import os

import numpy as np
import pytest

import lpgen
import update_cases as UC
import update_matrix_cases as MC
from highs_amd import abi, solver
from highs_amd import lp as L

GOLD = os.path.join(os.path.dirname(__file__), "golden")
CTEST = ["25fv47", "adlittle", "afiro", "avgas", "blending", "chip", "e226", "scrs8", "sctest", "shell", "stair",
         "standata", "standgub"]
MAKERS = {name: (lambda name=name: L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz"))) for name in CTEST}
MAKERS["structured_lp"] = lambda: lpgen.structured_lp()
MAKERS["random_diag_qp"] = lambda: lpgen.random_diag_qp(3)
MAKERS["random_sparse_qp"] = lambda: lpgen.random_sparse_qp(3)
ARRAYS = ("csr_beg", "csr_idx", "csr_val", "csc_beg", "csc_idx", "csc_val", "cost", "rhs", "lower", "upper", "col_scale",
          "row_scale", "row_kind", "row_new_idx")
SCALARS = ("n", "m", "n_eqs", "n_orig", "nnz", "norm_cost", "norm_rhs", "mat_norm_inf", "spmv_blocks_ax", "spmv_blocks_aty")

_cache = {}


def _lp(name):
    if name not in _cache:
        _cache[name] = MAKERS[name]()
    return _cache[name]


def _fields(F):
    n, m, nnz = F.n, F.m, F.nnz
    size = dict(csr_beg=m + 1, csr_idx=nnz, csr_val=nnz, csc_beg=n + 1, csc_idx=nnz, csc_val=nnz, cost=n, rhs=m, lower=n,
                upper=n, col_scale=n, row_scale=m, row_kind=m, row_new_idx=m)
    g = lambda p, k: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].copy()
    out = {k: g(getattr(F, k), size[k]) for k in ARRAYS}
    out.update({k: getattr(F, k) for k in SCALARS})
    return out


def _prepare(lp, **options):
    lib = solver.lib()
    P = abi.ProblemHandle(lp)
    params = abi.default_params(**options)
    F = abi.PdlpPrepared()
    assert lib.pdlp_mi355x_host_prepare(C.byref(P.struct), C.byref(params), C.byref(F)) == 0, lib.pdlp_mi355x_last_error().decode()
    out = _fields(F)
    lib.pdlp_mi355x_free_prepared(C.byref(F))
    return out


def _prepare_updated_matrix(lp, a_value, u=None, then=None, **options):
    """(rc, fields or the message): host_prepare_updated_matrix[_then] on lp."""
    lib = solver.lib()
    P = abi.ProblemHandle(lp)
    options.setdefault("updatable", "matrix")
    params = abi.default_params(**options)
    F = abi.PdlpPrepared()
    a = None if a_value is None else np.ascontiguousarray(a_value, dtype=np.float64)
    pa = None if a is None else a.ctypes.data_as(abi.c_f64p)
    pu = None if u is None else C.byref(u.struct)
    if then is None:
        rc = lib.pdlp_mi355x_host_prepare_updated_matrix(C.byref(P.struct), C.byref(params), pa, pu, C.byref(F))
    else:
        rc = lib.pdlp_mi355x_host_prepare_updated_matrix_then(C.byref(P.struct), C.byref(params), pa, pu, C.byref(then.struct), C.byref(F))
    if rc != 0:
        return rc, lib.pdlp_mi355x_last_error().decode()
    out = _fields(F)
    lib.pdlp_mi355x_free_prepared(C.byref(F))
    return 0, out


def _assert_same_fields(got, want):
    for k in ARRAYS:
        assert got[k].shape == want[k].shape and np.array_equal(got[k], want[k]), k
    for k in SCALARS:
        assert got[k] == want[k], (k, got[k], want[k])


def _data_handle(u):
    data = {k: v for k, v in u.items() if k != "a_value"}
    return abi.UpdateHandle(**data) if data else None


def _assert_update_equals_fresh(lp, u, **options):
    rc, got = _prepare_updated_matrix(lp, u["a_value"], _data_handle(u), **options)
    assert rc == 0, got
    _assert_same_fields(got, _prepare(MC.apply(lp, u), **options))


def test_the_symbols_exist():
    lib = solver.lib()
    for name in ("pdlp_mi355x_update_matrix", "pdlp_mi355x_host_prepare_updated_matrix"):
        assert hasattr(lib, name), name


@pytest.mark.parametrize("what", MC.KINDS)
@pytest.mark.parametrize("name", CTEST + ["structured_lp", "random_diag_qp"])
def test_matrix_update_equals_fresh_prepare(name, what):
    lp = _lp(name)
    _assert_update_equals_fresh(lp, MC.modification(lp, what, seed=len(name) + 13))


def test_the_values_really_move_the_scale_factors():
    """The cases are no no-ops: the matrix, both scale vectors and the scaled cost all differ from those of P."""
    lp = _lp("25fv47")
    u = MC.modification(lp, "values", seed=19)
    before, after = _prepare(lp), _prepare(MC.apply(lp, u))
    for k in ("csr_val", "csc_val", "col_scale", "row_scale", "cost", "rhs"):
        assert not np.array_equal(before[k], after[k]), k
    assert np.array_equal(before["csr_idx"], after["csr_idx"]) and np.array_equal(before["csc_beg"], after["csc_beg"])
    assert np.count_nonzero(after["csr_val"] == 0.0) > 0  # explicit zeros stay entries


def test_matrix_update_equals_fresh_prepare_maximise():
    lp = copy.copy(_lp("e226"))
    lp.sense = -1
    _assert_update_equals_fresh(lp, MC.modification(lp, "all", seed=5))


@pytest.mark.parametrize("name", ["afiro", "25fv47", "random_diag_qp"])
def test_matrix_update_equals_fresh_prepare_without_scaling(name):
    lp = _lp(name)
    _assert_update_equals_fresh(lp, MC.modification(lp, "all", seed=11), pdlp_features_off=abi.FEATURE_SCALING_OFF)


def test_unchanged_values_change_nothing():
    lp = _lp("25fv47")
    _assert_update_equals_fresh(lp, dict(a_value=np.array(lp.a_value)))


@pytest.mark.parametrize("name", ["25fv47", "scrs8", "structured_lp", "random_diag_qp"])
def test_matrix_update_then_update_replays_the_new_factors(name):
    """update_matrix(a', u1), then update(u2) on the same form = host_prepare of the twice-modified problem; the second
    step only divides by kept factors, so it matches only if those are the factors of a'."""
    lp = _lp(name)
    u1 = MC.modification(lp, "all", seed=23)
    lp1 = MC.apply(lp, u1)
    u2 = UC.modification(lp1, "all", seed=29)
    rc, got = _prepare_updated_matrix(lp, u1["a_value"], _data_handle(u1), then=abi.UpdateHandle(**u2))
    assert rc == 0, got
    _assert_same_fields(got, _prepare(UC.apply(lp1, u2)))
    # ... and with the factors of the ORIGINAL matrix the data would differ
    rc, stale = _prepare_updated_matrix(lp, np.array(lp.a_value), None, then=abi.UpdateHandle(**u2))
    assert rc == 0 and not np.array_equal(stale["cost"], got["cost"])


def test_through_the_python_wrapper():
    lp = _lp("adlittle")
    u = MC.modification(lp, "all", seed=31)
    got = solver.Prepared(lp, updatable="matrix", update_matrix=(u["a_value"], _data_handle(u)))
    want = solver.Prepared(MC.apply(lp, u))
    for k in ("csr_val", "csc_val", "cost", "rhs", "lower", "upper", "col_scale", "row_scale"):
        assert np.array_equal(getattr(got, k), getattr(want, k)), k
    assert got.mat_norm_inf == want.mat_norm_inf


# ---- refusals that need no solver handle -------------------------------------------------------------------------
def _refused(lp, a_value, u=None, **options):
    rc, msg = _prepare_updated_matrix(lp, a_value, u, **options)
    assert rc != 0
    return msg


def test_refuses_a_solver_not_created_for_matrix_updates():
    lp = _lp("afiro")
    for flag in (False, True):  # updatable = 0 and PDLP_UPDATABLE_DATA alone
        msg = _refused(lp, lp.a_value, updatable=flag)
        assert "pdlp_mi355x_update_matrix" in msg and "PDLP_UPDATABLE_MATRIX" in msg


def test_refuses_hipdlp():
    lp = _lp("afiro")
    msg = _refused(lp, lp.a_value, solver="hipdlp")
    assert "HiPDLP" in msg and "algorithm = 1" in msg


def test_refuses_an_off_diagonal_hessian():
    lp = _lp("random_sparse_qp")
    msg = _refused(lp, lp.a_value)
    assert "off-diagonal" in msg and "Hessian" in msg


def test_refuses_null_values():
    lp = _lp("afiro")
    assert "a_value is NULL" in _refused(lp, None)


def test_refuses_an_all_zero_matrix_with_the_wording_of_create():
    lp = _lp("afiro")
    msg = _refused(lp, np.zeros(len(lp.a_value)))
    zero = copy.copy(lp)
    zero.a_value = np.zeros(len(lp.a_value))
    with pytest.raises(RuntimeError) as e:  # (create refuses before it touches a device)
        solver.DeviceSolver(zero)
    assert msg in str(e.value) and "no matrix nonzeros" in msg


def test_refuses_what_update_refuses():
    lp = _lp("25fv47")
    a = MC.new_values(lp, 3)
    assert "row_upper is NULL" in _refused(lp, a, abi.UpdateHandle(row_lower=lp.row_lower))
    assert "partial start" in _refused(lp, a, abi.UpdateHandle(start=dict(col_value=np.zeros(lp.num_col))))
    kind = UC.row_kind(np.asarray(lp.row_lower), np.asarray(lp.row_upper))
    eq = np.nonzero(kind == 0)[0]
    lo, up = np.array(lp.row_lower), np.array(lp.row_upper)
    rows = sorted(int(i) for i in (eq[eq.size // 3], eq[-1]))
    for i in rows:
        up[i] = lo[i] + 1.0  # equality -> ranged
    msg = _refused(lp, a, abi.UpdateHandle(col_cost=lp.col_cost, row_lower=lo, row_upper=up))
    assert f"row {rows[0]} " in msg and "equality" in msg and "ranged or free" in msg


def test_refuses_a_null_solver():
    lib = solver.lib()
    a = np.ones(3)
    assert lib.pdlp_mi355x_update_matrix(None, a.ctypes.data_as(abi.c_f64p), 3, None) != 0
    assert "null solver" in lib.pdlp_mi355x_last_error().decode()


# ---- ABI: what this change must not move ---------------------------------------------------------------------------
def test_abi_numbers_stay():
    lib = solver.lib()
    assert lib.pdlp_mi355x_abi_version() == 6
    assert lib.pdlp_mi355x_sizeof(1) == C.sizeof(abi.PdlpParams) == 104
    assert lib.pdlp_mi355x_sizeof(8) == C.sizeof(abi.PdlpUpdate)
    assert lib.pdlp_mi355x_sizeof(9) == -1


def test_updatable_values():
    assert abi.default_params().updatable == 0
    assert abi.default_params(updatable=True).updatable == 1 and abi.default_params(updatable=1).updatable == 1
    assert abi.default_params(updatable="matrix").updatable == 3
    assert abi.default_params(updatable=abi.UPDATABLE_DATA | abi.UPDATABLE_MATRIX).updatable == 3
    assert abi.default_params(updatable=abi.UPDATABLE_MATRIX).updatable == 3  # MATRIX implies DATA
    assert (abi.UPDATABLE_DATA, abi.UPDATABLE_MATRIX) == (1, 2)
