"""The 64-bit column-start entries on the device (pdlp_mi355x_create_wide / pdlp_mi355x_solve_wide).  The device path
still has 32-bit offsets (problems above INT32_MAX nonzeros are refused), so what is checked here is the interface: the
starts that reach the device are a_start64, never P->a_start — every call below hands the library a DECOY P->a_start
(all -1: malformed, the 32-bit entries refuse it) — and with them a problem solves exactly as through the 32-bit entries (every
solution vector and the iteration, trial and restart counts; the device state after a fixed number of iterations), bit
for bit.  The refusals above INT32_MAX end the call with their message on a machine with a GPU as well."""
import ctypes as C
import os

import numpy as np
import pytest

import lpgen
from highs_amd import abi, solver
from highs_amd import lp as L

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CTEST = ["25fv47", "adlittle", "afiro", "avgas", "blending", "chip", "e226", "scrs8", "sctest", "shell", "stair",
         "standata", "standgub"]
OPTIONS = dict(kkt_tolerance=1e-4, pdlp_iteration_limit=20000)


def _decoy(n):
    """A P->a_start the wide entries must not read (kept alive by the caller)."""
    return np.full(n + 1, -1, np.int32)


def _solve_wide(lp, **options):
    """pdlp_mi355x_solve_wide with lp's starts as int64 (values below INT32_MAX: solveLpCupdlp would take the 32-bit entry)."""
    P = abi.ProblemHandle(lp)
    starts = np.ascontiguousarray(lp.a_start, dtype=np.int64)
    decoy = _decoy(lp.num_col)
    P.struct.a_start = decoy.ctypes.data_as(abi.c_i32p)
    R = abi.ResultHandle(lp.num_col, lp.num_row)
    params = abi.default_params(**options)
    rc = solver.lib().pdlp_mi355x_solve_wide(C.byref(P.struct), starts.ctypes.data_as(abi.c_i64p), C.byref(params),
                                             C.byref(R.struct))
    assert rc == 0, solver.lib().pdlp_mi355x_last_error().decode()
    return R


def _assert_same_solve(lp):
    narrow = solver.solveLpCupdlp(lp, **OPTIONS).result
    wide = _solve_wide(lp, **OPTIONS)
    for k in ("col_value", "col_dual", "row_value", "row_dual"):
        assert np.array_equal(getattr(narrow, k), getattr(wide, k)), k
    for k in ("term_code", "num_iter", "num_trials", "num_restarts"):
        assert getattr(narrow, k) == getattr(wide, k), k
    assert narrow.primal_obj == wide.primal_obj and narrow.dual_obj == wide.dual_obj


@pytest.mark.parametrize("name", CTEST)
def test_wide_entry_solves_ctest_instances_bit_for_bit(name):
    _assert_same_solve(L.HighsLp.from_npz(os.path.join(GOLD, "instances", name + ".npz")))


@pytest.mark.parametrize("make", [
    lambda: lpgen.structured_lp(),  # device-side set-up (>= 200k nonzeros)
    lambda: lpgen.random_diag_qp(3),
    lambda: lpgen.random_sparse_qp(3),
], ids=["structured_lp", "random_diag_qp", "random_sparse_qp"])
def test_wide_entry_solves_generated_problems_bit_for_bit(make):
    _assert_same_solve(make())


def test_wide_entry_iterates_bench_config_a_bit_for_bit():
    """bench.py config a: the device state after 200 iterations of a solver made by create_wide and by create."""
    sp_ = solver.SyntheticProblem(100_000, 100_000, 1_000_000, 1)
    P = sp_.struct
    starts = np.ctypeslib.as_array(P.a_start, shape=(P.num_col + 1,)).astype(np.int64)
    wideP = abi.PdlpProblem.from_buffer_copy(P)
    decoy = _decoy(P.num_col)
    wideP.a_start = decoy.ctypes.data_as(abi.c_i32p)
    params = abi.default_params(kkt_tolerance=1e-4)
    Lib = solver.lib()
    state = {}
    for kind in ("narrow", "wide"):
        h = C.c_void_p()
        if kind == "narrow":
            rc = Lib.pdlp_mi355x_create(C.byref(P), C.byref(params), C.byref(h))
        else:
            rc = Lib.pdlp_mi355x_create_wide(C.byref(wideP), starts.ctypes.data_as(abi.c_i64p), C.byref(params), C.byref(h))
        assert rc == 0, Lib.pdlp_mi355x_last_error().decode()
        try:
            dims = [C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()]
            assert Lib.pdlp_mi355x_dims(h, *[C.byref(d) for d in dims]) == 0
            nf, mf = dims[0].value, dims[1].value
            st = abi.PdlpIterStats()
            assert Lib.pdlp_mi355x_iterate(h, 200, C.byref(st)) == 0, Lib.pdlp_mi355x_last_error().decode()
            out = {"dims": tuple(d.value for d in dims), "iters": (st.iters, st.trials, st.restarts)}
            for name, length in (("x", nf), ("y", mf), ("ax", mf), ("aty", nf)):
                v = np.zeros(length)
                assert Lib.pdlp_mi355x_get_vector(h, name.encode(), v.ctypes.data_as(abi.c_f64p), length) == 0
                out[name] = v
            state[kind] = out
        finally:
            Lib.pdlp_mi355x_destroy(h)
    a, b = state["narrow"], state["wide"]
    assert a["dims"] == b["dims"] and a["iters"] == b["iters"]
    for name in ("x", "y", "ax", "aty"):
        assert np.array_equal(a[name], b[name]), name


@pytest.mark.parametrize("options, message", [
    (dict(solver="hipdlp"), "the HiPDLP path (algorithm = 1) takes at most INT32_MAX"),
    (dict(num_devices=2), "sharded solves (num_devices > 1) take at most INT32_MAX"),
    ({}, "the device path indexes the formulated matrix with 32-bit offsets"),
])
def test_wide_refusals_end_the_call_with_their_message(options, message, monkeypatch):
    """No device work starts for a problem above INT32_MAX; num_devices = 2 folded onto one GPU as the sharded tests do."""
    monkeypatch.setenv("PDLP_MI355X_FOLD_DEVICES", "1")
    big = 2**31 + 5
    lp = L.HighsLp(num_col=2, num_row=3, col_cost=np.ones(2), col_lower=np.zeros(2), col_upper=np.ones(2),
                   row_lower=np.zeros(3), row_upper=np.full(3, 2.0), a_start=np.array([0, 1, big], np.int64),
                   a_index=np.array([0, 1, 2], np.int32), a_value=np.ones(3))
    params = abi.default_params(**{k: v for k, v in options.items() if k != "num_devices"})
    params.num_devices = options.get("num_devices", 1)
    out = solver.solveLpCupdlp(lp, params=params)
    assert out.status == solver.kError
    assert message in solver.lib().pdlp_mi355x_last_error().decode()
