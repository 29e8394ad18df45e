"""The device-resident entries (pdlp_mi355x_create_device, _update_device, _run_device) on a machine without a GPU: the
symbols exist and change nothing of the ABI, null arguments and everything that needs no device are refused before any HIP
call in the host entries' words behind the new names, and tensors.TensorProblem checks dtype, layout and device in
Python.  What the entries compute is in tests/test_gpu_resident.py."""
import ctypes as C
import os

import numpy as np
import pytest

from highs_amd import abi, solver
from highs_amd import lp as L

GOLD = os.path.join(os.path.dirname(__file__), "golden")
NAMES = ("pdlp_mi355x_create_device", "pdlp_mi355x_update_device", "pdlp_mi355x_run_device")
# pdlp_mi355x_sizeof(0..8) as the four host tests that pin ABI version 6 see them
SIZES = [C.sizeof(t) for t in (abi.PdlpProblem, abi.PdlpParams, abi.PdlpResult, abi.PdlpIterStats, abi.PdlpPrepared,
                               abi.PdlpSlabLayout, abi.PdlpMpsModel, abi.PdlpTaskPlan, abi.PdlpUpdate)]


def _err():
    return solver.lib().pdlp_mi355x_last_error().decode()


def _afiro():
    return L.HighsLp.from_npz(os.path.join(GOLD, "instances", "afiro.npz"))


def test_the_three_symbols_exist_and_are_listed():
    lib = solver.lib()
    for name in NAMES:
        assert hasattr(lib, name), name
        assert name in solver.EXPORTS, name


def test_abi_version_and_struct_sizes_are_unchanged():
    lib = solver.lib()
    assert lib.pdlp_mi355x_abi_version() == 6
    assert [lib.pdlp_mi355x_sizeof(i) for i in range(9)] == SIZES
    assert lib.pdlp_mi355x_sizeof(9) == -1


def test_null_arguments_are_refused_with_a_message():
    lib = solver.lib()
    P = abi.ProblemHandle(_afiro())
    opt = abi.default_params()
    h = C.c_void_p()
    U = abi.PdlpUpdate()
    R = abi.PdlpResult()
    assert lib.pdlp_mi355x_create_device(None, C.byref(opt), None, C.byref(h)) != 0
    assert _err() == "pdlp_mi355x_create_device: null argument"
    assert lib.pdlp_mi355x_create_device(C.byref(P.struct), None, None, C.byref(h)) != 0
    assert _err() == "pdlp_mi355x_create_device: null argument"
    assert lib.pdlp_mi355x_create_device(C.byref(P.struct), C.byref(opt), None, None) != 0
    assert _err() == "pdlp_mi355x_create_device: null argument"
    assert lib.pdlp_mi355x_update_device(None, None, 0, None, 0, C.byref(U), None) != 0
    assert _err() == "pdlp_mi355x_update_device: null solver"
    assert lib.pdlp_mi355x_run_device(None, C.byref(R)) != 0
    assert _err() == "pdlp_mi355x_run_device: null solver"
    assert not h.value


@pytest.mark.parametrize("options, words", [
    (dict(solver="hipdlp"), "HiPDLP solvers (algorithm = 1) do not take updates"),
    (dict(num_devices=2), "sharded solvers (more than one device) do not take updates"),
])
def test_create_device_refuses_what_is_out_of_scope_before_any_device_call(options, words):
    # (host arrays in the struct: the refusal comes before the pointer check, and that before any launch)
    P = abi.ProblemHandle(_afiro())
    opt = abi.default_params(**options)
    h = C.c_void_p()
    assert solver.lib().pdlp_mi355x_create_device(C.byref(P.struct), C.byref(opt), None, C.byref(h)) != 0
    assert _err() == "pdlp_mi355x_create_device: " + words
    assert not h.value


def test_create_device_refuses_forced_sharding(monkeypatch):
    monkeypatch.setenv("PDLP_MI355X_FORCE_COMM", "1")
    P = abi.ProblemHandle(_afiro())
    opt = abi.default_params()
    h = C.c_void_p()
    assert solver.lib().pdlp_mi355x_create_device(C.byref(P.struct), C.byref(opt), None, C.byref(h)) != 0
    assert _err() == "pdlp_mi355x_create_device: sharded solvers (sharding forced) do not take updates"


@pytest.mark.parametrize("field, words", [
    ("col_cost", "null column arrays"), ("a_start", "null column arrays"), ("row_upper", "null row arrays"),
    ("a_value", "null matrix arrays"),  # a count with a NULL array
])
def test_create_device_refuses_a_missing_array_in_creates_words(field, words):
    P = abi.ProblemHandle(_afiro())
    setattr(P.struct, field, None)
    opt = abi.default_params()
    h = C.c_void_p()
    assert solver.lib().pdlp_mi355x_create_device(C.byref(P.struct), C.byref(opt), None, C.byref(h)) != 0
    assert _err() == "pdlp_mi355x_create_device: " + words
    # the host entry's words for the same struct
    assert solver.lib().pdlp_mi355x_create(C.byref(P.struct), C.byref(opt), C.byref(h)) != 0
    assert _err() == words


def _refusal(lp, updatable, a_value=None, num_nz=None, q_value=None, num_q_nz=None, **update):
    """pdlp_mi355x_host_update_device_refusal: what update_device refuses before any HIP call for a solver created on lp."""
    P = abi.ProblemHandle(lp)
    opt = abi.default_params(updatable=updatable) if updatable else abi.default_params()
    U = abi.UpdateHandle(**update)
    a = None if a_value is None else np.ascontiguousarray(a_value, dtype=np.float64)
    q = None if q_value is None else np.ascontiguousarray(q_value, dtype=np.float64)
    rc = solver.lib().pdlp_mi355x_host_update_device_refusal(
        C.byref(P.struct), C.byref(opt), None if a is None else a.ctypes.data_as(abi.c_f64p),
        (0 if a is None else a.size) if num_nz is None else num_nz, None if q is None else q.ctypes.data_as(abi.c_f64p),
        (0 if q is None else q.size) if num_q_nz is None else num_q_nz, C.byref(U.struct))
    return rc, _err()


def _host_words(lp, updatable, a_value=None, u=None):
    """The host entries' words for the same refusal, from the host restatements of update / update_matrix."""
    P = abi.ProblemHandle(lp)
    opt = abi.default_params(updatable=updatable) if updatable else abi.default_params()
    U = abi.UpdateHandle(**(u or {}))
    prep = abi.PdlpPrepared()
    if a_value is None:
        rc = solver.lib().pdlp_mi355x_host_prepare_updated(C.byref(P.struct), C.byref(opt), C.byref(U.struct), C.byref(prep))
    else:
        a = np.ascontiguousarray(a_value, dtype=np.float64)
        rc = solver.lib().pdlp_mi355x_host_prepare_updated_matrix(C.byref(P.struct), C.byref(opt), a.ctypes.data_as(abi.c_f64p),
                                                                  C.byref(U.struct), C.byref(prep))
    words = _err()
    solver.lib().pdlp_mi355x_free_prepared(C.byref(prep))
    assert rc != 0
    return words


def test_update_device_refuses_row_bounds_that_are_not_a_pair():
    lp = _afiro()
    u = dict(row_lower=lp.row_lower)
    rc, words = _refusal(lp, True, **u)
    assert rc != 0
    assert words == "pdlp_mi355x_update_device: " + _host_words(lp, True, u=u)
    assert "row_lower and row_upper are given together or not at all (row_upper is NULL)" in words


def test_update_device_refuses_a_start_that_is_not_whole():
    lp = _afiro()
    u = dict(start=dict(col_value=np.zeros(lp.num_col), row_dual=np.zeros(lp.num_row)))
    rc, words = _refusal(lp, True, **u)
    assert rc != 0
    assert words == "pdlp_mi355x_update_device: " + _host_words(lp, True, u=u)
    assert "partial start" in words and "2 of 3 are given" in words
    # ... on the matrix route as well
    rc, words = _refusal(lp, "matrix", a_value=lp.a_value, **u)
    assert rc != 0 and words == "pdlp_mi355x_update_device: " + _host_words(lp, "matrix", a_value=lp.a_value, u=u)


def test_update_device_refuses_a_count_with_a_null_array():
    lp = _afiro()
    rc, words = _refusal(lp, "matrix+hessian", num_nz=lp.a_value.size)
    assert rc != 0
    assert words == "pdlp_mi355x_update_device: pdlp_mi355x_update_values: a_value is NULL but num_nz = %d" % lp.a_value.size
    rc, words = _refusal(lp, "matrix+hessian", num_q_nz=3)
    assert rc != 0
    assert words == "pdlp_mi355x_update_device: pdlp_mi355x_update_values: q_value is NULL but num_q_nz = 3"
    # without the Hessian bit a count alone goes to update_values too, which asks for the bit first
    rc, words = _refusal(lp, "matrix", num_nz=lp.a_value.size)
    assert rc != 0 and words.startswith("pdlp_mi355x_update_device: pdlp_mi355x_update_values: the solver was not created for Hessian updates")


def test_update_device_routes_and_refuses_by_the_updatable_bits():
    lp = _afiro()
    rc, words = _refusal(lp, None, col_cost=lp.col_cost)
    assert rc != 0 and words == "pdlp_mi355x_update_device: " + _host_words(lp, None, u=dict(col_cost=lp.col_cost))
    assert "not created for updates" in words
    rc, words = _refusal(lp, True, a_value=lp.a_value)
    assert rc != 0 and words == "pdlp_mi355x_update_device: " + _host_words(lp, True, a_value=lp.a_value)
    assert "lacks PDLP_UPDATABLE_MATRIX" in words
    rc, words = _refusal(lp, "matrix", a_value=lp.a_value[:-1])
    assert rc != 0 and "num_nz = %d differs from the %d nonzeros" % (lp.a_value.size - 1, lp.a_value.size) in words
    # what is in order is not refused
    assert _refusal(lp, True, col_cost=lp.col_cost, row_lower=lp.row_lower, row_upper=lp.row_upper)[0] == 0
    assert _refusal(lp, "matrix", a_value=lp.a_value, col_cost=lp.col_cost)[0] == 0


# ---- tensors.TensorProblem, with CPU tensors only -----------------------------------------------------------------------
def _cpu_fields(lp):
    torch = pytest.importorskip("torch")
    f64 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64).copy())
    i32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32).copy())
    return dict(num_col=lp.num_col, num_row=lp.num_row, col_cost=f64(lp.col_cost), col_lower=f64(lp.col_lower),
                col_upper=f64(lp.col_upper), row_lower=f64(lp.row_lower), row_upper=f64(lp.row_upper), a_start=i32(lp.a_start),
                a_index=i32(lp.a_index), a_value=f64(lp.a_value), sense=lp.sense, offset=lp.offset)


def test_tensor_problem_rejects_cpu_tensors():
    from highs_amd import tensors as T
    with pytest.raises(ValueError, match="a_start: a tensor on a cuda device is needed"):
        T.TensorProblem(**_cpu_fields(_afiro()))


def test_tensor_problem_rejects_wrong_dtypes():
    from highs_amd import tensors as T
    f = _cpu_fields(_afiro())
    f["a_start"] = f["a_start"].long()
    with pytest.raises(TypeError, match="a_start: dtype torch.int32 is needed, got torch.int64"):
        T.TensorProblem(**f)
    f = _cpu_fields(_afiro())
    f["a_start"] = f["a_start"].numpy()
    with pytest.raises(TypeError, match="a_start: a torch tensor is needed, got ndarray"):
        T.TensorProblem(**f)
    import torch
    with pytest.raises(TypeError, match="col_cost: dtype torch.float64 is needed, got torch.float32"):
        T.check_tensor("col_cost", torch.zeros(4, dtype=torch.float32), "float64")


def test_tensor_problem_rejects_non_contiguous_tensors():
    import torch

    from highs_amd import tensors as T
    f = _cpu_fields(_afiro())
    wide = torch.zeros(2 * f["a_start"].numel(), dtype=torch.int32)
    f["a_start"] = wide[::2]
    with pytest.raises(ValueError, match="a_start: a contiguous tensor is needed"):
        T.TensorProblem(**f)
    with pytest.raises(ValueError, match="x: a one-dimensional tensor is needed"):
        T.check_tensor("x", torch.zeros(2, 2, dtype=torch.float64), "float64")
