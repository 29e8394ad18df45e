"""CPU tests of the 64-bit column-start entries (pdlp_mi355x_create_wide / pdlp_mi355x_solve_wide): the library checks
a_start64 on the host before any HIP call, so every malformed input and every refusal below is reported the same with or
without a GPU; and highs_amd.solver sends an int64 start array with values above INT32_MAX to the wide entry.  Nothing
here allocates 2^31 entries: a refusal is decided from the starts alone."""
import ctypes as C

import numpy as np
import pytest

from highs_amd import abi, solver
from highs_amd.lp import HighsLp

BIG = 2**31 + 5  # one column with more than INT32_MAX entries


def _lp(a_start, a_index, num_row=3):
    n = len(a_start) - 1
    return HighsLp(num_col=n, num_row=num_row, col_cost=np.ones(n), col_lower=np.zeros(n), col_upper=np.ones(n),
                   row_lower=np.zeros(num_row), row_upper=np.full(num_row, 2.0), a_start=np.asarray(a_start, np.int64),
                   a_index=np.asarray(a_index, np.int32), a_value=np.ones(len(a_index)))


def _wide_call(entry, lp, a_start64, num_nz=None, **params):
    """rc and last_error of pdlp_mi355x_create_wide (entry = "create") or pdlp_mi355x_solve_wide ("solve")."""
    P = abi.ProblemHandle(lp)
    P.struct.a_start = None
    P.struct.num_nz = int(a_start64[-1]) if num_nz is None else num_nz
    starts = np.ascontiguousarray(a_start64, dtype=np.int64)
    opt = abi.default_params(**params)
    L = solver.lib()
    if entry == "create":
        h = C.c_void_p()
        rc = L.pdlp_mi355x_create_wide(C.byref(P.struct), starts.ctypes.data_as(abi.c_i64p), C.byref(opt), C.byref(h))
        if h:
            L.pdlp_mi355x_destroy(h)
    else:
        R = abi.ResultHandle(lp.num_col, lp.num_row)
        rc = L.pdlp_mi355x_solve_wide(C.byref(P.struct), starts.ctypes.data_as(abi.c_i64p), C.byref(opt), C.byref(R.struct))
    return rc, L.pdlp_mi355x_last_error().decode()


GOOD_START, GOOD_INDEX = [0, 2, 3, 5], [0, 2, 1, 0, 1]


@pytest.mark.parametrize("entry", ["create", "solve"])
@pytest.mark.parametrize("starts, index, num_nz, message", [
    ([1, 2, 3, 5], GOOD_INDEX, 5, "a_start64[0] must be 0, is 1"),
    ([0, 3, 2, 5], GOOD_INDEX, 5, "a_start64 decreases at column 1: a_start64[1] = 3, a_start64[2] = 2"),
    ([0, 2, 3, 5], GOOD_INDEX, 6, "a_start64[num_col] = 5 differs from num_nz = 6"),
    ([0, 2, 3, 5], [0, 2, 1, 3, 1], 5, "row index out of range"),
    ([0, 2, 3, 5], [0, -1, 1, 0, 1], 5, "row index out of range"),
])
def test_malformed_starts_are_reported_before_any_device_call(entry, starts, index, num_nz, message):
    rc, err = _wide_call(entry, _lp(GOOD_START, index), starts, num_nz=num_nz)
    assert rc != 0
    assert message in err, err


@pytest.mark.parametrize("entry", ["create", "solve"])
def test_null_starts_are_an_error(entry):
    lp = _lp(GOOD_START, GOOD_INDEX)
    P = abi.ProblemHandle(lp)
    opt = abi.default_params()
    L = solver.lib()
    if entry == "create":
        h = C.c_void_p()
        rc = L.pdlp_mi355x_create_wide(C.byref(P.struct), None, C.byref(opt), C.byref(h))
    else:
        R = abi.ResultHandle(lp.num_col, lp.num_row)
        rc = L.pdlp_mi355x_solve_wide(C.byref(P.struct), None, C.byref(opt), C.byref(R.struct))
    assert rc != 0 and "null argument" in L.pdlp_mi355x_last_error().decode()


@pytest.mark.parametrize("entry, params, message", [
    ("create", {}, "the device path indexes the formulated matrix with 32-bit offsets"),
    ("solve", {}, "the device path indexes the formulated matrix with 32-bit offsets"),
    ("create", {"solver": "hipdlp"}, "the HiPDLP path (algorithm = 1) takes at most INT32_MAX"),
    ("solve", {"solver": "hipdlp"}, "the HiPDLP path (algorithm = 1) takes at most INT32_MAX"),
])
def test_more_than_int32_max_nonzeros_are_refused_by_name(entry, params, message):
    rc, err = _wide_call(entry, _lp([0, BIG], [0, 1, 2]), [0, BIG], **params)
    assert rc != 0
    assert message in err and "this problem has %d nonzeros" % BIG in err, err


def test_sharded_solve_of_more_than_int32_max_nonzeros_is_refused():
    lp = _lp([0, BIG], [0, 1, 2])
    rc, err = _wide_call("solve", lp, [0, BIG], num_devices=2)
    assert rc != 0
    assert "sharded solves (num_devices > 1) take at most INT32_MAX" in err, err


@pytest.mark.parametrize("entry", ["create", "solve"])
def test_p_a_start_is_not_read(entry):
    """a_start64 replaces P->a_start: a malformed P->a_start next to valid 64-bit starts passes the host checks (the call
    then ends at the device: a solver on a GPU box, "no HIP device" without one)."""
    lp = _lp(GOOD_START, GOOD_INDEX)
    P = abi.ProblemHandle(lp)
    decoy = np.full(lp.num_col + 1, -1, np.int32)
    P.struct.a_start = decoy.ctypes.data_as(abi.c_i32p)
    starts = np.asarray(GOOD_START, np.int64)
    opt = abi.default_params(pdlp_iteration_limit=10)
    L = solver.lib()
    if entry == "create":
        h = C.c_void_p()
        rc = L.pdlp_mi355x_create_wide(C.byref(P.struct), starts.ctypes.data_as(abi.c_i64p), C.byref(opt), C.byref(h))
        if h:
            L.pdlp_mi355x_destroy(h)
    else:
        R = abi.ResultHandle(lp.num_col, lp.num_row)
        rc = L.pdlp_mi355x_solve_wide(C.byref(P.struct), starts.ctypes.data_as(abi.c_i64p), C.byref(opt), C.byref(R.struct))
    assert rc == 0 or "no HIP device" in L.pdlp_mi355x_last_error().decode(), L.pdlp_mi355x_last_error().decode()


def _fake(calls, name):
    """A stand-in entry that records its arguments and fails: the mirror then computes no KKT measures (which would walk
    the 2^31 entries the starts promise)."""
    def fn(*args):
        calls.append((name, args))
        return 1
    return fn


def test_int64_starts_above_int32_max_take_the_wide_entry():
    calls = []
    lp = _lp([0, 1, BIG], [0, 1, 2])
    solver.solveLpCupdlp(lp, solve_fn=_fake(calls, "narrow"), solve_wide_fn=_fake(calls, "wide"))
    assert [c[0] for c in calls] == ["wide"]
    P, starts = calls[0][1][0]._obj, calls[0][1][1]
    assert not P.a_start and P.num_nz == BIG
    assert [starts[j] for j in range(3)] == [0, 1, BIG]


def test_int64_starts_that_fit_take_the_narrow_entry():
    calls = []
    lp = _lp(GOOD_START, GOOD_INDEX)
    assert lp.a_start.dtype == np.int64
    solver.solveLpCupdlp(lp, solve_fn=_fake(calls, "narrow"), solve_wide_fn=_fake(calls, "wide"))
    assert [c[0] for c in calls] == ["narrow"]
    P = calls[0][1][0]._obj
    assert [P.a_start[j] for j in range(4)] == GOOD_START and P.num_nz == 5


def test_hipdlp_mirror_passes_wide_starts_on():
    calls = []
    solver.solveLpHiPdlp(_lp([0, 1, BIG], [0, 1, 2]), solve_fn=_fake(calls, "narrow"), solve_wide_fn=_fake(calls, "wide"))
    assert [c[0] for c in calls] == ["wide"]
    assert calls[0][1][2]._obj.algorithm == 1


def test_a_narrow_stand_in_does_not_take_wide_starts():
    with pytest.raises(ValueError, match="pass solve_wide_fn"):
        solver.solveLpCupdlp(_lp([0, 1, BIG], [0, 1, 2]), solve_fn=_fake([], "narrow"))


@pytest.mark.parametrize("mirror, message", [
    (solver.solveLpCupdlp, "32-bit offsets"),
    (solver.solveLpHiPdlp, "HiPDLP path (algorithm = 1)"),
])
def test_mirrors_report_the_library_refusal(mirror, message):
    out = mirror(_lp([0, 1, BIG], [0, 1, 2]))
    assert out.status == solver.kError and out.model_status == solver.kSolveError
    assert message in solver.lib().pdlp_mi355x_last_error().decode()
