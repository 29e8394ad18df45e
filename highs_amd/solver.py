"""Host-side mirror of the reference interface of the PDLP path.

`solveLpCupdlp(lp, options)` has the role of the reference's
`HighsStatus solveLpCupdlp(HighsLpSolverObject&)` (highs/pdlp/CupdlpWrapper.cpp:23-278):
options in (`getUserParamsFromOptions` :642-717), HighsSolution / model status
/ pdlp_iteration_count out (status map :225-251).  All the arithmetic happens
in the C-ABI library libpdlp_mi355x.so on the GPU; there is NO CPU fallback —
if the library or a HIP device is missing this raises.
"""
import ctypes as C
import os
import subprocess
from dataclasses import dataclass, field

import numpy as np

from . import abi
from .lp import HighsLp, kkt_measures

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "lib", "libpdlp_mi355x.so")
if os.environ.get("PDLP_MI355X_LIB"):  # development: an experimental build of the same library
    LIB_PATH = os.environ["PDLP_MI355X_LIB"]

# HighsModelStatus values (lp_data/HConst.h, highs_c_api.h:74-91)
kSolveError, kOptimal, kInfeasible, kUnboundedOrInfeasible, kUnbounded = 4, 7, 8, 9, 10
kTimeLimit, kIterationLimit, kUnknown = 13, 14, 15
MODEL_STATUS_NAME = {4: "Solve error", 7: "Optimal", 8: "Infeasible", 9: "Primal infeasible or unbounded",
                     10: "Unbounded", 13: "Time limit reached", 14: "Iteration limit reached", 15: "Unknown"}
# HighsStatus
kOk, kWarning, kError = 0, 1, -1

_lib = None

EXPORTS = [
    "pdlp_mi355x_default_params", "pdlp_mi355x_solve", "pdlp_mi355x_create", "pdlp_mi355x_run",
    "pdlp_mi355x_destroy", "pdlp_mi355x_dims", "pdlp_mi355x_reset", "pdlp_mi355x_iterate",
    "pdlp_mi355x_get_vector", "pdlp_mi355x_set_vector", "pdlp_mi355x_stage", "pdlp_mi355x_time_kernel",
    "pdlp_mi355x_comm_unique_id", "pdlp_mi355x_create_sharded", "pdlp_mi355x_gen_synthetic",
    "pdlp_mi355x_free_problem", "pdlp_mi355x_last_error", "pdlp_mi355x_abi_version",
    "pdlp_mi355x_host_prepare", "pdlp_mi355x_free_prepared", "pdlp_mi355x_row_partition", "pdlp_mi355x_sizeof",
    "pdlp_mi355x_host_slab_layout", "pdlp_mi355x_free_slab_layout", "pdlp_mi355x_det_exp_log",
    "pdlp_mi355x_host_task_plan", "pdlp_mi355x_free_task_plan",
    "pdlp_mi355x_read_mps", "pdlp_mi355x_read_mps_timed", "pdlp_mi355x_free_mps_model",
    "pdlp_mi355x_create_wide", "pdlp_mi355x_solve_wide",
    "pdlp_mi355x_update", "pdlp_mi355x_host_prepare_updated",
    "pdlp_mi355x_update_matrix", "pdlp_mi355x_host_prepare_updated_matrix",
    "pdlp_mi355x_update_values", "pdlp_mi355x_host_prepare_qp", "pdlp_mi355x_free_prepared_hessian",
    "pdlp_mi355x_session_create", "pdlp_mi355x_session_solve", "pdlp_mi355x_session_info", "pdlp_mi355x_session_release",
    "pdlp_mi355x_session_destroy", "pdlp_mi355x_session_info_size", "pdlp_mi355x_host_classify",
    "pdlp_mi355x_batch_create", "pdlp_mi355x_batch_run", "pdlp_mi355x_batch_info", "pdlp_mi355x_batch_destroy",
    "pdlp_mi355x_batch_info_size", "pdlp_mi355x_batch_run_values", "pdlp_mi355x_variant_size",
    "pdlp_mi355x_solve_many", "pdlp_mi355x_pool_info_size",
    "pdlp_mi355x_create_device", "pdlp_mi355x_update_device", "pdlp_mi355x_run_device",
    "pdlp_mi355x_batch_run_device",
]


def build(force=False):
    """Compile the HIP library for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force and os.path.exists(LIB_PATH):
        os.remove(LIB_PATH)
    subprocess.check_call(["make", "-s", "-C", src])
    return LIB_PATH


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                               "(the PDLP path has no CPU fallback)")
        L = C.CDLL(LIB_PATH)
        # One HIP runtime per process (tensors.py): a PyTorch wheel bundles a libamdhip64 of its own and asks for it by the
        # name "libamdhip64.so".  Registering the copy this library has just brought in under that name makes a LATER
        # `import torch` bind to it instead of loading a second runtime, which would find no device (or leave this one
        # without).  With torch imported first the library has bound to torch's copy already; without torch this is a no-op.
        try:
            C.CDLL("libamdhip64.so", mode=C.RTLD_GLOBAL)
        except OSError:
            pass
        pP, pO, pR = C.POINTER(abi.PdlpProblem), C.POINTER(abi.PdlpParams), C.POINTER(abi.PdlpResult)
        H = C.c_void_p
        L.pdlp_mi355x_default_params.argtypes = [pO]
        L.pdlp_mi355x_solve.argtypes = [pP, pO, pR]
        L.pdlp_mi355x_create.argtypes = [pP, pO, C.POINTER(H)]
        L.pdlp_mi355x_solve_wide.argtypes = [pP, abi.c_i64p, pO, pR]
        L.pdlp_mi355x_create_wide.argtypes = [pP, abi.c_i64p, pO, C.POINTER(H)]
        L.pdlp_mi355x_create_sharded.argtypes = [pP, pO, C.c_int32, C.c_int32, C.c_void_p, C.POINTER(H)]
        L.pdlp_mi355x_run.argtypes = [H, pR]
        L.pdlp_mi355x_destroy.argtypes = [H]
        L.pdlp_mi355x_destroy.restype = None
        L.pdlp_mi355x_dims.argtypes = [H, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32)]
        L.pdlp_mi355x_reset.argtypes = [H]
        L.pdlp_mi355x_iterate.argtypes = [H, C.c_int32, C.POINTER(abi.PdlpIterStats)]
        L.pdlp_mi355x_get_vector.argtypes = [H, C.c_char_p, abi.c_f64p, C.c_int64]
        L.pdlp_mi355x_set_vector.argtypes = [H, C.c_char_p, abi.c_f64p, C.c_int64]
        L.pdlp_mi355x_stage.argtypes = [H, C.c_char_p, abi.c_f64p, C.c_int32]
        L.pdlp_mi355x_time_kernel.argtypes = [H, C.c_char_p, C.c_int32, C.POINTER(C.c_double)]
        L.pdlp_mi355x_comm_unique_id.argtypes = [C.c_void_p]
        L.pdlp_mi355x_gen_synthetic.argtypes = [C.c_int32, C.c_int32, C.c_int64, C.c_uint64, pP]
        L.pdlp_mi355x_free_problem.argtypes = [pP]
        L.pdlp_mi355x_free_problem.restype = None
        pPrep = C.POINTER(abi.PdlpPrepared)
        L.pdlp_mi355x_host_prepare.argtypes = [pP, pO, pPrep]
        L.pdlp_mi355x_free_prepared.argtypes = [pPrep]
        pU = C.POINTER(abi.PdlpUpdate)
        L.pdlp_mi355x_update.argtypes = [H, pU]
        L.pdlp_mi355x_host_prepare_updated.argtypes = [pP, pO, pU, pPrep]
        L.pdlp_mi355x_update_matrix.argtypes = [H, abi.c_f64p, C.c_int64, pU]
        L.pdlp_mi355x_host_prepare_updated_matrix.argtypes = [pP, pO, abi.c_f64p, pU, pPrep]
        # (a test hook outside the public header: host_prepare_updated_matrix with a data update behind it)
        L.pdlp_mi355x_host_prepare_updated_matrix_then.argtypes = [pP, pO, abi.c_f64p, pU, pU, pPrep]
        L.pdlp_mi355x_free_prepared.restype = None
        pQ = C.POINTER(abi.PdlpPreparedHessian)
        L.pdlp_mi355x_update_values.argtypes = [H, abi.c_f64p, C.c_int64, abi.c_f64p, C.c_int64, pU]
        L.pdlp_mi355x_host_prepare_qp.argtypes = [pP, pO, abi.c_f64p, abi.c_f64p, pU, pPrep, pQ]
        # (a test hook outside the public header: host_prepare_qp with a data update behind it)
        L.pdlp_mi355x_host_prepare_qp_then.argtypes = [pP, pO, abi.c_f64p, abi.c_f64p, pU, pU, pPrep, pQ]
        L.pdlp_mi355x_free_prepared_hessian.argtypes = [pQ]
        L.pdlp_mi355x_free_prepared_hessian.restype = None
        pI = C.POINTER(abi.PdlpSessionInfo)
        L.pdlp_mi355x_session_create.argtypes = [C.POINTER(H)]
        L.pdlp_mi355x_session_solve.argtypes = [H, pP, pO, pR]
        L.pdlp_mi355x_session_info.argtypes = [H, pI]
        L.pdlp_mi355x_session_release.argtypes = [H]
        L.pdlp_mi355x_session_release.restype = None
        L.pdlp_mi355x_session_destroy.argtypes = [H]
        L.pdlp_mi355x_session_destroy.restype = None
        L.pdlp_mi355x_session_info_size.restype = C.c_int64
        L.pdlp_mi355x_host_classify.argtypes = [pP, pO, pP, pO, pI]
        if L.pdlp_mi355x_session_info_size() != C.sizeof(abi.PdlpSessionInfo):
            raise RuntimeError("pdlp_session_info_t: the library's size %d differs from abi.PdlpSessionInfo's %d" %
                               (L.pdlp_mi355x_session_info_size(), C.sizeof(abi.PdlpSessionInfo)))
        # (a build from before the batches, given through PDLP_MI355X_LIB, has none: tools/batch_bench.py's sequential side)
        if hasattr(L, "pdlp_mi355x_batch_create"):
            pB = C.POINTER(abi.PdlpBatchInfo)
            L.pdlp_mi355x_batch_create.argtypes = [pP, pO, C.c_int32, C.POINTER(H)]
            L.pdlp_mi355x_batch_run.argtypes = [H, C.c_int32, pU, pR]
            # (a build from before the value variants has neither: tools/batch_values_bench.py's sequential side)
            if hasattr(L, "pdlp_mi355x_batch_run_values"):
                pV = C.POINTER(abi.PdlpVariant)
                L.pdlp_mi355x_batch_run_values.argtypes = [H, C.c_int32, pV, pR]
                L.pdlp_mi355x_variant_size.restype = C.c_int64
                # (a test hook outside the public header: batch_run_values' refusals that need no device)
                L.pdlp_mi355x_host_batch_variants_refusal.argtypes = [pP, pO, C.c_int32, pV, pR]
                if L.pdlp_mi355x_variant_size() != C.sizeof(abi.PdlpVariant):
                    raise RuntimeError("pdlp_variant_t: the library's size %d differs from abi.PdlpVariant's %d" %
                                       (L.pdlp_mi355x_variant_size(), C.sizeof(abi.PdlpVariant)))
            # (a build from before the device batches has none of these: tools/batch_resident_bench.py's parent side)
            if hasattr(L, "pdlp_mi355x_batch_run_device"):
                L.pdlp_mi355x_batch_run_device.argtypes = [H, C.c_int32, pV, pR, C.c_void_p]
                # (test hooks outside the public header: batch_run_device's refusals that need no device, its verdict on
                # canned records of the validation launch, and that launch alone)
                L.pdlp_mi355x_host_batch_device_variants_refusal.argtypes = [pP, pO, C.c_int32, pV, pR]
                L.pdlp_mi355x_host_batch_records_verdict.argtypes = [C.c_int32, pV, abi.c_i32p, abi.c_i32p, C.c_int32, C.c_int32]
                L.pdlp_mi355x_batch_variant_records.argtypes = [H, C.c_int32, pV, C.c_int32, abi.c_i32p]
            L.pdlp_mi355x_batch_info.argtypes = [H, pB]
            L.pdlp_mi355x_batch_destroy.argtypes = [H]
            L.pdlp_mi355x_batch_destroy.restype = None
            L.pdlp_mi355x_batch_info_size.restype = C.c_int64
            if L.pdlp_mi355x_batch_info_size() != C.sizeof(abi.PdlpBatchInfo):
                raise RuntimeError("pdlp_batch_info_t: the library's size %d differs from abi.PdlpBatchInfo's %d" %
                                   (L.pdlp_mi355x_batch_info_size(), C.sizeof(abi.PdlpBatchInfo)))
        # (likewise a build from before the pools: tools/pool_bench.py's sequential side)
        if hasattr(L, "pdlp_mi355x_solve_many"):
            L.pdlp_mi355x_solve_many.argtypes = [C.c_int32, C.POINTER(pP), pO, C.c_int32, pR, abi.c_i32p, C.POINTER(abi.PdlpPoolInfo)]
            L.pdlp_mi355x_pool_info_size.restype = C.c_int64
            if L.pdlp_mi355x_pool_info_size() != C.sizeof(abi.PdlpPoolInfo):
                raise RuntimeError("pdlp_pool_info_t: the library's size %d differs from abi.PdlpPoolInfo's %d" %
                                   (L.pdlp_mi355x_pool_info_size(), C.sizeof(abi.PdlpPoolInfo)))
        # (a build from before the device-resident entries, given through PDLP_MI355X_LIB: tools/resident_bench.py's host side)
        if hasattr(L, "pdlp_mi355x_create_device"):
            L.pdlp_mi355x_create_device.argtypes = [pP, pO, C.c_void_p, C.POINTER(H)]
            L.pdlp_mi355x_update_device.argtypes = [H, abi.c_f64p, C.c_int64, abi.c_f64p, C.c_int64, pU, C.c_void_p]
            L.pdlp_mi355x_run_device.argtypes = [H, pR]
            # (a test hook outside the public header: update_device's refusals that need no device)
            L.pdlp_mi355x_host_update_device_refusal.argtypes = [pP, pO, abi.c_f64p, C.c_int64, abi.c_f64p, C.c_int64, pU]
        L.pdlp_mi355x_row_partition.argtypes = [pPrep, C.c_int32, abi.c_i32p]
        pSlab = C.POINTER(abi.PdlpSlabLayout)
        L.pdlp_mi355x_host_slab_layout.argtypes = [pPrep, C.c_int32, C.c_int32, pSlab]
        L.pdlp_mi355x_free_slab_layout.argtypes = [pSlab]
        L.pdlp_mi355x_free_slab_layout.restype = None
        pTask = C.POINTER(abi.PdlpTaskPlan)
        L.pdlp_mi355x_host_task_plan.argtypes = [pPrep, C.c_int32, C.c_int32, C.c_int32, pTask]
        L.pdlp_mi355x_free_task_plan.argtypes = [pTask]
        L.pdlp_mi355x_free_task_plan.restype = None
        # (a test hook outside the public header: the stream layout's work plan)
        pPlan = C.POINTER(abi.PdlpStreamPlan)
        L.pdlp_mi355x_host_stream_plan.argtypes = [pPrep, C.c_int32, C.c_int32, C.c_int32, pPlan]
        L.pdlp_mi355x_free_stream_plan.argtypes = [pPlan]
        L.pdlp_mi355x_free_stream_plan.restype = None
        # (a test hook outside the public header: what a solver holds of an operand after its set-up)
        if hasattr(L, "pdlp_mi355x_device_matrix"):  # (an older build given through PDLP_MI355X_LIB has none)
            pDevM = C.POINTER(abi.PdlpDeviceMatrix)
            L.pdlp_mi355x_device_matrix.argtypes = [H, C.c_int32, pDevM]
            L.pdlp_mi355x_free_device_matrix.argtypes = [pDevM]
            L.pdlp_mi355x_free_device_matrix.restype = None
        pMps = C.POINTER(abi.PdlpMpsModel)
        L.pdlp_mi355x_read_mps.argtypes = [C.c_char_p, C.c_int32, pMps]
        L.pdlp_mi355x_read_mps_timed.argtypes = [C.c_char_p, C.c_int32, C.c_double, pMps]
        L.pdlp_mi355x_free_mps_model.argtypes = [pMps]
        L.pdlp_mi355x_free_mps_model.restype = None
        L.pdlp_mi355x_det_exp_log.argtypes = [C.c_int32, abi.c_f64p, abi.c_f64p, abi.c_f64p]
        L.pdlp_mi355x_det_exp_log.restype = None
        L.pdlp_mi355x_sizeof.argtypes = [C.c_int32]
        L.pdlp_mi355x_sizeof.restype = C.c_int64
        L.pdlp_mi355x_last_error.restype = C.c_char_p
        L.pdlp_mi355x_abi_version.restype = C.c_int
        _lib = L
    return _lib


def _check(rc, what):
    if rc != 0:
        raise RuntimeError(f"{what} failed: {lib().pdlp_mi355x_last_error().decode()}")


class MpsFixedFormat(RuntimeError):
    """The file has names with spaces: a fixed-column reader is needed (return code 3 of pdlp_mi355x_read_mps)."""


class MpsTimeout(RuntimeError):
    """options.time_limit passed while the file was read (return code 5: FilereaderRetcode::kTimeout)."""


def read_mps(path, threads=0, time_limit=0.0):
    """Highs::readModel for an MPS file through the library's multi-threaded reader (csrc/pdlp_mps.cpp; the
    reference: io/FilereaderMps.cpp:24-58 -> io/HMpsFF.cpp).  Returns (HighsLp, info); info carries what HighsLp
    has no field for: integrality, names, objective name, cost row location, warnings, threads, seconds.
    time_limit: HMpsFF::time_limit_ (seconds; <= 0: none)."""
    M = abi.PdlpMpsModel()
    L = lib()
    rc = L.pdlp_mi355x_read_mps_timed(os.fsencode(path), int(threads), float(time_limit), C.byref(M))
    if rc == 2:
        raise FileNotFoundError(L.pdlp_mi355x_last_error().decode())
    if rc == 3:
        raise MpsFixedFormat(L.pdlp_mi355x_last_error().decode())
    if rc == 5:
        raise MpsTimeout(L.pdlp_mi355x_last_error().decode())
    _check(rc, "pdlp_mi355x_read_mps")
    try:
        P = M.lp
        n, m, nz = P.num_col, P.num_row, P.num_nz
        arr = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(k,)).astype(dt).copy() if k else np.zeros(0, dt)
        lp = HighsLp(n, m, arr(P.col_cost, n, np.float64), arr(P.col_lower, n, np.float64), arr(P.col_upper, n, np.float64),
                     arr(P.row_lower, m, np.float64), arr(P.row_upper, m, np.float64),
                     np.ctypeslib.as_array(P.a_start, shape=(n + 1,)).astype(np.int32).copy(),
                     arr(P.a_index, nz, np.int32), arr(P.a_value, nz, np.float64), P.sense, P.offset,
                     (M.model_name or b"").decode())
        if P.q_dim > 0:
            qs = np.ctypeslib.as_array(P.q_start, shape=(P.q_dim + 1,)).astype(np.int32).copy()
            lp.hessian = (qs, arr(P.q_index, int(qs[-1]), np.int32), arr(P.q_value, int(qs[-1]), np.float64))

        def names(pool, start, k):
            if not start or k == 0:
                return None
            st = np.ctypeslib.as_array(start, shape=(k + 1,))
            raw = C.string_at(pool, int(st[k]))
            return [raw[int(st[i]):int(st[i + 1]) - 1].decode() for i in range(k)]

        info = dict(cost_row_location=M.cost_row_location, objective_name=(M.objective_name or b"").decode(),
                    integrality=arr(M.integrality, M.num_integrality, np.uint8) if M.num_integrality else None,
                    col_names=names(M.col_name_pool, M.col_name_start, n), row_names=names(M.row_name_pool, M.row_name_start, m),
                    num_warnings=M.num_warnings, warning_issued=bool(M.warning_issued), warnings=(M.warnings or b"").decode().splitlines(), threads=M.threads,
                    file_bytes=M.file_bytes, seconds=M.seconds)
        if M.hessian_dim > 0:
            hs = np.ctypeslib.as_array(M.hessian_start, shape=(M.hessian_dim + 1,)).astype(np.int32).copy()
            info["hessian_square"] = (hs, arr(M.hessian_index, int(hs[-1]), np.int32), arr(M.hessian_value, int(hs[-1]), np.float64))
        return lp, info
    finally:
        L.pdlp_mi355x_free_mps_model(C.byref(M))


@dataclass
class HighsSolution:
    col_value: np.ndarray
    col_dual: np.ndarray
    row_value: np.ndarray
    row_dual: np.ndarray
    value_valid: bool = False
    dual_valid: bool = False


@dataclass
class PdlpOutcome:
    status: int  # HighsStatus
    model_status: int  # HighsModelStatus
    solution: HighsSolution
    pdlp_iteration_count: int
    info: dict = field(default_factory=dict)
    result: object = None


def model_status_from_term(term_code, num_iter, iter_limit, rc=0):
    """Status map of CupdlpWrapper.cpp:225-251."""
    if rc != 0:
        return kSolveError
    if term_code == abi.TERM_OPTIMAL:
        return kOptimal
    if term_code == abi.TERM_INFEASIBLE:
        return kInfeasible
    if term_code == abi.TERM_UNBOUNDED:
        return kUnbounded
    if term_code == abi.TERM_INFEASIBLE_OR_UNBOUNDED:
        return kUnboundedOrInfeasible
    if term_code == abi.TERM_TIMELIMIT_OR_ITERLIMIT:
        return kIterationLimit if num_iter >= iter_limit - 1 else kTimeLimit
    return kUnknown


def _solve_once(P, params, R, solve_fn, solve_wide_fn):
    """pdlp_mi355x_solve, or pdlp_mi355x_solve_wide when the column starts go beyond INT32_MAX (abi.ProblemHandle.wide).
    solve_fn / solve_wide_fn stand in for the two entries."""
    if not P.wide:
        return (solve_fn or lib().pdlp_mi355x_solve)(C.byref(P.struct), C.byref(params), C.byref(R.struct))
    if solve_fn is not None and solve_wide_fn is None:
        raise ValueError("the column starts go beyond INT32_MAX: solve_fn takes 32-bit starts, pass solve_wide_fn")
    fn = solve_wide_fn or lib().pdlp_mi355x_solve_wide
    return fn(C.byref(P.struct), P.a_start.ctypes.data_as(abi.c_i64p), C.byref(params), C.byref(R.struct))


def _outcome(lp, R, params, rc):
    ms = model_status_from_term(R.term_code, R.num_iter, params.iter_limit, rc)
    sol = HighsSolution(R.col_value, R.col_dual, R.row_value, R.row_dual, bool(R.value_valid), bool(R.dual_valid))
    info = kkt_measures(lp, sol.col_value, sol.col_dual, sol.row_value, sol.row_dual) if rc == 0 else {}
    info["pdlp_iteration_count"] = int(R.num_iter)
    status = kError if rc != 0 else (kOk if ms == kOptimal or ms == kUnboundedOrInfeasible else kWarning)
    return PdlpOutcome(status, ms, sol, int(R.num_iter), info, R)


class Session:
    """pdlp_mi355x_session_*: one resident solver reused across whole-problem solves.  Every solve() takes a whole HighsLp,
    as solveLpCupdlp does; the library finds on the device what differs from the problem it holds and creates, updates or
    forwards accordingly (include/pdlp_mi355x.h has the ladder).  One thread at a time."""

    def __init__(self):
        self.h = C.c_void_p()
        _check(lib().pdlp_mi355x_session_create(C.byref(self.h)), "pdlp_mi355x_session_create")

    def solve(self, lp, start=None, **options):
        """-> (PdlpOutcome as solveLpCupdlp returns it, abi.PdlpSessionInfo).  A failed solve is reported through the
        outcome's status (kError / kSolveError), as solveLpCupdlp reports it; the session then holds nothing."""
        params = options.pop("params", None) or abi.default_params(**options)
        P = abi.ProblemHandle(lp, start)
        if P.wide:
            raise ValueError("sessions take 32-bit column starts")
        R = abi.ResultHandle(lp.num_col, lp.num_row)
        rc = lib().pdlp_mi355x_session_solve(self.h, C.byref(P.struct), C.byref(params), C.byref(R.struct))
        out = _outcome(lp, R, params, rc)
        if rc != 0:
            out.info["error"] = lib().pdlp_mi355x_last_error().decode()
        return out, self.info

    @property
    def info(self):
        """About the last solve (path NONE before the first)."""
        I = abi.PdlpSessionInfo()
        _check(lib().pdlp_mi355x_session_info(self.h, C.byref(I)), "pdlp_mi355x_session_info")
        return I

    def release(self):
        """Drop the held solver; the session stays usable (the next solve creates)."""
        lib().pdlp_mi355x_session_release(self.h)

    def close(self):
        if self.h:
            lib().pdlp_mi355x_session_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_classify(lp_held, lp, held_options=None, start=None, **options):
    """pdlp_mi355x_host_classify: what a session holding lp_held (solved with held_options; lp_held None: holding nothing)
    would do with lp and **options -> abi.PdlpSessionInfo.  Host only."""
    held_params = abi.default_params(**(held_options or {}))
    params = abi.default_params(**options)
    H = None if lp_held is None else abi.ProblemHandle(lp_held)
    P = abi.ProblemHandle(lp, start)
    I = abi.PdlpSessionInfo()
    _check(lib().pdlp_mi355x_host_classify(None if H is None else C.byref(H.struct), C.byref(held_params), C.byref(P.struct),
                                           C.byref(params), C.byref(I)), "pdlp_mi355x_host_classify")
    return I


def solveLpCupdlp(lp: HighsLp, start=None, solve_fn=None, solve_wide_fn=None, session=None, **options):
    """Solve `lp` with the MI355X PDLP path.  Keyword options use the HiGHS
    option names: kkt_tolerance, primal_feasibility_tolerance (primal_tol),
    pdlp_iteration_limit, pdlp_features_off, time_limit, log_level, ...
    An int64 `lp.a_start` with values above INT32_MAX goes through pdlp_mi355x_solve_wide.
    `solve_fn` lets the tests run the same marshalling against the oracle; `solve_wide_fn`
    stands in for the wide entry the same way.  `session`: a Session — the solve goes through it (pdlp_mi355x_session_solve)
    and reuses the solver it holds where the problem allows; session.info tells which path was taken."""
    if session is not None:
        return session.solve(lp, start=start, **options)[0]
    params = options.pop("params", None) or abi.default_params(**options)
    P = abi.ProblemHandle(lp, start)
    R = abi.ResultHandle(lp.num_col, lp.num_row)
    rc = _solve_once(P, params, R, solve_fn, solve_wide_fn)
    ms = model_status_from_term(R.term_code, R.num_iter, params.iter_limit, rc)
    sol = HighsSolution(R.col_value, R.col_dual, R.row_value, R.row_dual, bool(R.value_valid), bool(R.dual_valid))
    info = kkt_measures(lp, sol.col_value, sol.col_dual, sol.row_value, sol.row_dual) if rc == 0 else {}
    info["pdlp_iteration_count"] = int(R.num_iter)
    status = kError if rc != 0 else (kOk if ms == kOptimal or ms == kUnboundedOrInfeasible else kWarning)
    return PdlpOutcome(status, ms, sol, int(R.num_iter), info, R)


def run_model_file(path, solver="pdlp", threads=0, **options):
    """Highs::readModel + Highs::run with solver="pdlp" / "hipdlp" and presolve off, on this package's side of the C
    ABI: the library's MPS reader (read_mps), then the solve.  Returns (PdlpOutcome, HighsLp, read info)."""
    lp, info = read_mps(path, threads)
    if info["integrality"] is not None and info["integrality"].any():
        raise ValueError("the model has integer columns: solver=\"pdlp\" is for LPs (and diagonal QPs)")
    out = solveLpCupdlp(lp, **options) if solver == "pdlp" else solveLpHiPdlp(lp, **options)
    return out, lp, info


def solveLpHiPdlp(lp: HighsLp, solve_fn=None, solve_wide_fn=None, **options):
    """Mirror of the reference's second PDLP entry point, solveLpHiPdlp (highs/pdlp/HiPdlpWrapper.cpp:26-141):
    restarted Halpern PDHG.  Same option names as HiGHS (kkt_tolerance / pdlp_optimality_tolerance ->
    gap_tol, pdlp_iteration_limit, time_limit, pdlp_features_off, pdlp_scaling_mode, pdlp_ruiz_iterations,
    pdlp_step_size_strategy); status map of HiPdlpWrapper.cpp:99-128.  Column starts above INT32_MAX go to
    pdlp_mi355x_solve_wide as in solveLpCupdlp (which refuses them on this path)."""
    options = dict(options)
    options["solver"] = "hipdlp"
    params = options.pop("params", None) or abi.default_params(**options)
    P = abi.ProblemHandle(lp)
    R = abi.ResultHandle(lp.num_col, lp.num_row)
    rc = _solve_once(P, params, R, solve_fn, solve_wide_fn)
    if rc != 0:
        ms = kSolveError
    elif R.term_code == abi.TERM_OPTIMAL:
        ms = kOptimal
    elif R.term_code == abi.TERM_TIMELIMIT_OR_ITERLIMIT:
        ms = kTimeLimit if R.reserved_i == 1 else kIterationLimit
    else:
        ms = kUnknown
    sol = HighsSolution(R.col_value, R.col_dual, R.row_value, R.row_dual, bool(R.value_valid), bool(R.dual_valid))
    info = kkt_measures(lp, sol.col_value, sol.col_dual, sol.row_value, sol.row_dual) if rc == 0 else {}
    info["pdlp_iteration_count"] = int(R.num_iter)
    return PdlpOutcome(kError if rc != 0 else kOk, ms, sol, int(R.num_iter), info, R)


class DeviceSolver:
    """Long-lived solver context with the problem resident in HBM (pdlp_mi355x_create ... destroy)."""

    def __init__(self, lp=None, problem_struct=None, params=None, rank=0, world=1, unique_id=None, **options):
        self.params = params or abi.default_params(**options)
        self._keep = None
        self.lp = lp
        if problem_struct is None:
            self._keep = abi.ProblemHandle(lp)
            problem_struct = self._keep.struct
        self.h = C.c_void_p()
        if self._keep is not None and self._keep.wide:  # 64-bit column starts (create_sharded takes 32-bit ones only)
            if world > 1:
                raise ValueError("sharded solves take 32-bit column starts")
            rc = lib().pdlp_mi355x_create_wide(C.byref(problem_struct), self._keep.a_start.ctypes.data_as(abi.c_i64p),
                                               C.byref(self.params), C.byref(self.h))
        elif world > 1:
            rc = lib().pdlp_mi355x_create_sharded(C.byref(problem_struct), C.byref(self.params), rank, world,
                                                  unique_id, C.byref(self.h))
        else:
            rc = lib().pdlp_mi355x_create(C.byref(problem_struct), C.byref(self.params), C.byref(self.h))
        _check(rc, "pdlp_mi355x_create")
        n, m, nnz, ne = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        _check(lib().pdlp_mi355x_dims(self.h, C.byref(n), C.byref(m), C.byref(nnz), C.byref(ne)), "dims")
        self.n, self.m, self.nnz, self.n_eqs = n.value, m.value, nnz.value, ne.value

    def close(self):
        if self.h:
            lib().pdlp_mi355x_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def run(self, num_col, num_row):
        R = abi.ResultHandle(num_col, num_row)
        _check(lib().pdlp_mi355x_run(self.h, C.byref(R.struct)), "pdlp_mi355x_run")
        return R

    def reset(self):
        _check(lib().pdlp_mi355x_reset(self.h), "reset")

    def update(self, col_cost=None, col_lower=None, col_upper=None, row_lower=None, row_upper=None, offset=None, start=None):
        """pdlp_mi355x_update: new costs / column bounds / row bounds / offset for the held problem (None = unchanged) and
        the start of the next run (`start`: dict with col_value, row_value, row_dual, or None = cold start).  Needs a
        solver created with updatable=True; raises with the library's message when the update is refused (the solver is
        then unchanged).  When the solver was built from a HighsLp, self.lp follows (a copy), so solve() reports the KKT
        measures of the problem actually solved."""
        U = abi.UpdateHandle(col_cost, col_lower, col_upper, row_lower, row_upper, offset, start)
        _check(lib().pdlp_mi355x_update(self.h, C.byref(U.struct)), "pdlp_mi355x_update")
        if self.lp is not None:
            import copy
            lp = copy.copy(self.lp)
            for name, a in (("col_cost", col_cost), ("col_lower", col_lower), ("col_upper", col_upper),
                            ("row_lower", row_lower), ("row_upper", row_upper)):
                if a is not None:
                    setattr(lp, name, np.array(a, dtype=np.float64))
            if offset is not None:
                lp.offset = float(offset)
            self.lp = lp

    def update_matrix(self, a_value, col_cost=None, col_lower=None, col_upper=None, row_lower=None, row_upper=None, offset=None,
                      start=None):
        """pdlp_mi355x_update_matrix: new matrix values on the sparsity pattern the solver was created with (a_value in the
        positions of the problem's a_value; None is passed on as NULL and refused), together with new data and a start as
        update() takes them, as one change.  Needs a solver created with updatable="matrix"; raises with the library's
        message when refused (the solver is then unchanged).  self.lp follows as in update()."""
        data = (col_cost, col_lower, col_upper, row_lower, row_upper, offset, start)
        U = abi.UpdateHandle(*data) if any(d is not None for d in data) else None
        a = None if a_value is None else np.ascontiguousarray(a_value, dtype=np.float64)
        _check(lib().pdlp_mi355x_update_matrix(self.h, None if a is None else a.ctypes.data_as(abi.c_f64p), 0 if a is None else a.size,
                                               None if U is None else C.byref(U.struct)), "pdlp_mi355x_update_matrix")
        if self.lp is not None:
            import copy
            lp = copy.copy(self.lp)
            lp.a_value = a.copy()
            for name, v in (("col_cost", col_cost), ("col_lower", col_lower), ("col_upper", col_upper),
                            ("row_lower", row_lower), ("row_upper", row_upper)):
                if v is not None:
                    setattr(lp, name, np.array(v, dtype=np.float64))
            if offset is not None:
                lp.offset = float(offset)
            self.lp = lp

    def update_values(self, a_value=None, q_value=None, col_cost=None, col_lower=None, col_upper=None, row_lower=None,
                      row_upper=None, offset=None, start=None):
        """pdlp_mi355x_update_values: new Hessian values (q_value in the positions of the problem's Hessian values) and / or
        new matrix values (a_value, as update_matrix takes them), together with new data and a start as update() takes
        them, as one change.  None = unchanged.  Needs a solver created with updatable="hessian" (or "matrix+hessian" for
        a_value); raises with the library's message when refused (the solver is then unchanged).  self.lp follows as in
        update(), its hessian included."""
        data = (col_cost, col_lower, col_upper, row_lower, row_upper, offset, start)
        U = abi.UpdateHandle(*data) if any(d is not None for d in data) else None
        a = None if a_value is None else np.ascontiguousarray(a_value, dtype=np.float64)
        q = None if q_value is None else np.ascontiguousarray(q_value, dtype=np.float64)
        _check(lib().pdlp_mi355x_update_values(self.h, None if a is None else a.ctypes.data_as(abi.c_f64p), 0 if a is None else a.size,
                                               None if q is None else q.ctypes.data_as(abi.c_f64p), 0 if q is None else q.size,
                                               None if U is None else C.byref(U.struct)), "pdlp_mi355x_update_values")
        if self.lp is not None:
            import copy
            lp = copy.copy(self.lp)
            if a is not None:
                lp.a_value = a.copy()
            if q is not None:
                hess = lp.hessian
                lp.hessian = (hess[0], hess[1], q.copy())
            for name, v in (("col_cost", col_cost), ("col_lower", col_lower), ("col_upper", col_upper),
                            ("row_lower", row_lower), ("row_upper", row_upper)):
                if v is not None:
                    setattr(lp, name, np.array(v, dtype=np.float64))
            if offset is not None:
                lp.offset = float(offset)
            self.lp = lp

    # ---- problems, updates and solutions as tensors in HBM (tensors.py; include/pdlp_mi355x.h "device-resident entries") ----
    @classmethod
    def from_tensors(cls, tp, start=None, **options):
        """pdlp_mi355x_create_device: a solver for a tensors.TensorProblem, whose arrays are in HBM already.  Bit for bit
        the solver DeviceSolver(lp, **options) is for the same problem in numpy arrays.  start: dict with col_value,
        row_value, row_dual as tensors on tp's device, or None.  The library reads the tensors behind torch's current
        stream; they may be changed or freed once this returns."""
        import torch

        from . import tensors as T

        if not isinstance(tp, T.TensorProblem):
            raise TypeError("from_tensors: a tensors.TensorProblem is needed, got %s" % type(tp).__name__)
        self = cls.__new__(cls)
        given = options.pop("params", None)
        self.params = given or abi.default_params(**options)
        if given is None and "device" not in options:
            self.params.device = T.device_ordinal(tp.device)
        elif self.params.device != T.device_ordinal(tp.device):
            raise ValueError("from_tensors: the problem is on %s, the options ask for device %d" % (tp.device, self.params.device))
        T.init()
        self._keep = None
        self.lp = None
        self.h = C.c_void_p()
        P, keep = tp.struct(start)
        with torch.cuda.device(tp.device):
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib().pdlp_mi355x_create_device(C.byref(P), C.byref(self.params), C.c_void_p(stream), C.byref(self.h))
        del keep
        _check(rc, "pdlp_mi355x_create_device")
        n, m, nnz, ne = C.c_int32(), C.c_int32(), C.c_int64(), C.c_int32()
        _check(lib().pdlp_mi355x_dims(self.h, C.byref(n), C.byref(m), C.byref(nnz), C.byref(ne)), "dims")
        self.n, self.m, self.nnz, self.n_eqs = n.value, m.value, nnz.value, ne.value
        self.num_col, self.num_row = tp.num_col, tp.num_row
        return self

    def _tensor_device(self):
        import torch

        return torch.device("cuda", self.params.device)

    def _tensor_sizes(self):
        if getattr(self, "num_col", None) is not None:
            return self.num_col, self.num_row
        if self.lp is not None:
            return self.lp.num_col, self.lp.num_row
        raise ValueError("the solver was built from a problem struct: set num_col and num_row on it first")

    def update_tensors(self, a_value=None, q_value=None, col_cost=None, col_lower=None, col_upper=None, row_lower=None,
                       row_upper=None, offset=None, start=None):
        """pdlp_mi355x_update_device: update() / update_matrix() / update_values() with every array a float64 tensor on the
        solver's device (None = unchanged; start: dict of three tensors or None = cold start).  Neither a_value nor q_value:
        a data update; a_value alone on a solver without updatable="...hessian": a matrix update; else a value update.  The
        tensors are read behind torch's current stream, without synchronising it, and may be changed once this returns.
        Raises with the library's message when the update is refused (the solver is then unchanged).  self.lp, a host
        copy, does not follow: read results with run_tensors()."""
        import torch

        from . import tensors as T

        dev = self._tensor_device()
        n0, m = self._tensor_sizes()
        if a_value is not None:
            T.check_tensor("a_value", a_value, "float64", None, dev)
        if q_value is not None:
            T.check_tensor("q_value", q_value, "float64", None, dev)
        U = T.TensorUpdate(n0, m, dev, col_cost, col_lower, col_upper, row_lower, row_upper, offset, start)
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream().cuda_stream
            rc = lib().pdlp_mi355x_update_device(self.h, T.pointer(a_value, abi.c_f64p), 0 if a_value is None else a_value.numel(),
                                                 T.pointer(q_value, abi.c_f64p), 0 if q_value is None else q_value.numel(),
                                                 C.byref(U.struct), C.c_void_p(stream))
        _check(rc, "pdlp_mi355x_update_device")

    def run_tensors(self, out=None):
        """pdlp_mi355x_run_device -> tensors.TensorResult: col_value, col_dual, row_value, row_dual as float64 tensors on
        the solver's device — those given in `out` (a dict by these names; a loop reuses its buffers), fresh ones
        otherwise — and the scalars of pdlp_result_t.  The tensors are complete when this returns.  With `out`, torch's
        current stream is synchronised first: work queued there may still read the previous solution from those tensors,
        and the library writes them on a stream of its own."""
        import torch

        from . import tensors as T

        n0, m = self._tensor_sizes()
        dev = self._tensor_device()
        R = T.TensorResult(n0, m, dev, out)
        with torch.cuda.device(dev):
            if out:  # (run_device takes no stream: what torch has queued that still reads the given tensors ends first)
                torch.cuda.current_stream().synchronize()
            rc = lib().pdlp_mi355x_run_device(self.h, C.byref(R.struct))
        _check(rc, "pdlp_mi355x_run_device")
        return R

    def solve(self):
        """pdlp_mi355x_run on the held problem, returned as solveLpCupdlp returns it: a family of LPs over one matrix
        is `create once; for each: update, solve`."""
        if self.lp is None:
            raise ValueError("solve() needs a solver built from a HighsLp (use run() with a problem struct)")
        lp = self.lp
        R = abi.ResultHandle(lp.num_col, lp.num_row)
        rc = lib().pdlp_mi355x_run(self.h, C.byref(R.struct))
        ms = model_status_from_term(R.term_code, R.num_iter, self.params.iter_limit, rc)
        sol = HighsSolution(R.col_value, R.col_dual, R.row_value, R.row_dual, bool(R.value_valid), bool(R.dual_valid))
        info = kkt_measures(lp, sol.col_value, sol.col_dual, sol.row_value, sol.row_dual) if rc == 0 else {}
        info["pdlp_iteration_count"] = int(R.num_iter)
        status = kError if rc != 0 else (kOk if ms == kOptimal or ms == kUnboundedOrInfeasible else kWarning)
        return PdlpOutcome(status, ms, sol, int(R.num_iter), info, R)

    def iterate(self, n_iters):
        st = abi.PdlpIterStats()
        _check(lib().pdlp_mi355x_iterate(self.h, n_iters, C.byref(st)), "iterate")
        return st

    def get(self, name, length):
        out = np.zeros(length)
        _check(lib().pdlp_mi355x_get_vector(self.h, name.encode(), out.ctypes.data_as(abi.c_f64p), length), "get " + name)
        return out

    def set(self, name, arr):
        arr = np.ascontiguousarray(arr, dtype=np.float64)
        _check(lib().pdlp_mi355x_set_vector(self.h, name.encode(), arr.ctypes.data_as(abi.c_f64p), arr.size), "set " + name)

    def stage(self, name, n_out=16, init=None):
        out = np.zeros(n_out)
        if init is not None:  # a few stages read their argument from the scalar array
            out[:len(init)] = init
        _check(lib().pdlp_mi355x_stage(self.h, name.encode(), out.ctypes.data_as(abi.c_f64p), n_out), "stage " + name)
        return out

    SETUP_SCALARS = ("norm_cost", "norm_rhs", "mat_norm_inf", "sum_cost2", "sum_rhs2", "n_eqs", "n0", "scaled", "gpu_setup")

    def setup_scalars(self):
        """Stage "setup_scalars" as a dict: what the set-up left on the host (NaN: this form has no such number) and
        gpu_setup, 1.0 where the device formulated, scaled and laid the problem out."""
        return dict(zip(self.SETUP_SCALARS, self.stage("setup_scalars", len(self.SETUP_SCALARS)).tolist()))

    HESSIAN_EXTRACTION = ("on_device", "reason", "taken_slots", "n_slots", "temp_bytes")

    def hessian_extraction(self):
        """Stage "hessian_extraction" as a dict: on_device 1.0 where the set-up extracted the Hessian on the device, the
        rule's reason code (HESSIAN_REASONS), the slots taken, the slots of N, the peak of the extraction's temporary HBM."""
        return dict(zip(self.HESSIAN_EXTRACTION, self.stage("hessian_extraction", len(self.HESSIAN_EXTRACTION)).tolist()))

    def hessian_map(self):
        """A Hessian-updatable solver's kept assembly map (read-only test hook): dst_beg [n + nOff + 1], src_slot, off_row,
        off_col [nOff] as int64 arrays."""
        n_off = int(self.hessian_extraction()["n_slots"])
        dst_beg = self.get("dstBeg", self.n + n_off + 1).astype(np.int64)
        return dict(dst_beg=dst_beg, src_slot=self.get("srcSlot", int(dst_beg[-1])).astype(np.int64),
                    off_row=self.get("offRow", n_off).astype(np.int64), off_col=self.get("offCol", n_off).astype(np.int64))

    def device_matrix(self, which):
        """pdlp_mi355x_device_matrix: what the solver holds of operand `which` (0: A by rows, 1: A' by columns), downloaded
        as it lies in HBM (no launch, no change of state).  A dict of numbers and numpy copies: beg / idx / val are the
        operand's CSR (stream layout) or the compact CSR of its long majors (slab layout); idx, val, ent and slab_val
        come with their pad element; blocks [n_blocks, 4], tasks [n_tasks, 8] (pdlp_task_plan_t's records)."""
        D = abi.PdlpDeviceMatrix()
        _check(lib().pdlp_mi355x_device_matrix(self.h, which, C.byref(D)), "device_matrix")
        g = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt).copy() if p else np.zeros(0, dtype=dt)
        nw = 16 * D.slab_blocks + 1 if D.use_slab else 0
        out = {k: getattr(D, k) for k in ("use_slab", "n_major", "n_minor", "nnz", "chunk", "n_blocks", "slab_blocks", "rows_per_block",
                                          "minor_bits", "slab_width_log2", "n_long", "n_tasks", "task_group", "long_group",
                                          "long_slots", "nnz_short", "tile_log2", "n_tiles")}
        out.update(
            beg=g(D.beg, D.n_csr_major + 1, np.int64), idx=g(D.idx, D.nnz_csr + 1, np.int64), val=g(D.val, D.nnz_csr + 1, np.float64),
            block_beg=g(D.block_beg, 4 * D.n_blocks, np.int64).reshape(-1, 4), tasks=g(D.tasks, 8 * D.n_tasks, np.int64).reshape(-1, 8),
            wave_beg=g(D.wave_beg, nw, np.int64), wave_ptr=g(D.wave_ptr, nw, np.int64),
            ent=g(D.ent, D.nnz_short + 1 if D.use_slab else 0, np.uint32), slab_val=g(D.slab_val, D.nnz_short + 1 if D.use_slab else 0, np.float64),
            long_mask=g(D.long_mask, D.n_mask_words, np.uint32), long_map=g(D.long_map, D.n_long if D.use_slab else 0, np.int64),
            tile_owner=g(D.tile_owner, D.n_tiles, np.int64), span_lo=g(D.span_lo, D.slab_blocks, np.int64),
            span_hi=g(D.span_hi, D.slab_blocks, np.int64), span_cnt=g(D.span_cnt, D.slab_blocks, np.int64))
        lib().pdlp_mi355x_free_device_matrix(C.byref(D))
        return out

    def time_kernel(self, name, reps=20):
        ms = C.c_double()
        _check(lib().pdlp_mi355x_time_kernel(self.h, name.encode(), reps, C.byref(ms)), "time " + name)
        return ms.value


class DeviceBatch:
    """pdlp_mi355x_batch_*: `lanes` (1..8) resident solvers of one LP; run() solves a list of variants of it — each a dict
    of DeviceSolver.update's arguments (col_cost, col_lower, col_upper, row_lower, row_upper, offset, start; {} = the LP as
    it is) plus, optionally, iter_limit for that variant alone — and returns one PdlpOutcome per variant, bit for bit what
    `DeviceSolver(lp, updatable=True, **options)` gives for update(**variant) + solve().  Where the LP's trial loop runs
    XCD-local the variants run at once, one per XCD (include/pdlp_mi355x.h; info().text says how the last run went).

    A variant's dict may also carry a_value= (new matrix values, for a batch created with updatable="matrix") and q_value=
    (new Hessian values, updatable="hessian" or "matrix+hessian"), each on the LP's own pattern; an array a variant leaves
    out is the LP's own, whatever variant its lane solved before.  If any variant has one, the call goes through
    pdlp_mi355x_batch_run_values, and the reference is `DeviceSolver(lp, updatable=…, **options)` (the batch's own
    `updatable`) + update_values(a_value, q_value, **data) — update_matrix(a_value, **data) for a_value alone on a batch
    without "hessian", update(**data) without either array — + solve()."""

    def __init__(self, lp, lanes=8, params=None, **options):
        self.params = params or abi.default_params(**options)
        self.lp = lp
        self._keep = abi.ProblemHandle(lp)
        if self._keep.wide:
            raise ValueError("batches take 32-bit column starts")
        self.h = C.c_void_p()
        _check(lib().pdlp_mi355x_batch_create(C.byref(self._keep.struct), C.byref(self.params), int(lanes), C.byref(self.h)),
               "pdlp_mi355x_batch_create")

    def run(self, variants):
        import copy
        K = len(variants)
        with_values = any(v.get("a_value") is not None or v.get("q_value") is not None for v in variants)
        handles, lps, limits = [], [], []
        U = ((abi.PdlpVariant if with_values else abi.PdlpUpdate) * max(K, 1))()
        Rs = (abi.PdlpResult * max(K, 1))()
        results = []
        for k, v in enumerate(variants):
            v = dict(v)
            limit = v.pop("iter_limit", None)
            a_value, q_value = v.pop("a_value", None), v.pop("q_value", None)
            hnd = abi.VariantHandle(a_value, q_value, **v) if with_values else abi.UpdateHandle(**v)
            if limit is not None:
                (hnd.struct.u if with_values else hnd.struct).reserved = int(limit)
            handles.append(hnd)
            U[k] = hnd.struct
            limits.append(self.params.iter_limit if limit is None else int(limit))
            lp = copy.copy(self.lp)
            for name in ("col_cost", "col_lower", "col_upper", "row_lower", "row_upper"):
                if v.get(name) is not None:
                    setattr(lp, name, np.array(v[name], dtype=np.float64))
            if v.get("offset") is not None:
                lp.offset = float(v["offset"])
            if a_value is not None:
                lp.a_value = np.array(a_value, dtype=np.float64)
            if q_value is not None:
                lp.hessian = (lp.hessian[0], lp.hessian[1], np.array(q_value, dtype=np.float64))
            lps.append(lp)
            R = abi.ResultHandle(self.lp.num_col, self.lp.num_row)
            results.append(R)
            Rs[k] = R.struct
        if with_values:
            _check(lib().pdlp_mi355x_batch_run_values(self.h, K, U, Rs), "pdlp_mi355x_batch_run_values")
        else:
            _check(lib().pdlp_mi355x_batch_run(self.h, K, U, Rs), "pdlp_mi355x_batch_run")
        out = []
        for k in range(K):
            results[k].struct = Rs[k]
            R, lp = results[k], lps[k]
            ms = model_status_from_term(R.term_code, R.num_iter, limits[k], 0)
            sol = HighsSolution(R.col_value, R.col_dual, R.row_value, R.row_dual, bool(R.value_valid), bool(R.dual_valid))
            info = kkt_measures(lp, sol.col_value, sol.col_dual, sol.row_value, sol.row_dual)
            info["pdlp_iteration_count"] = int(R.num_iter)
            status = kOk if ms == kOptimal or ms == kUnboundedOrInfeasible else kWarning
            out.append(PdlpOutcome(status, ms, sol, int(R.num_iter), info, R))
        return out

    # ---- variants and solutions as tensors in HBM (tensors.py; include/pdlp_mi355x.h pdlp_mi355x_batch_run_device) ----
    def _tensor_variants(self, variants):
        """-> (the pdlp_variant_t array, what keeps its tensors alive); TypeError / ValueError name the variant."""
        import torch

        from . import tensors as T

        dev = torch.device("cuda", self.params.device)
        V = (abi.PdlpVariant * max(len(variants), 1))()
        keep = []
        for k, v in enumerate(variants):
            unknown = set(v) - set(abi.VARIANT_KEYS)
            if unknown:
                raise ValueError(f"variants[{k}]: unknown keys {sorted(unknown)}; a variant takes {abi.VARIANT_KEYS}")
            try:
                tv = T.TensorVariant(self.lp.num_col, self.lp.num_row, dev, **v)
            except (TypeError, ValueError) as e:
                raise type(e)(f"variants[{k}]: {e}") from None
            keep.append(tv)
            V[k] = tv.struct
        return V, keep

    def run_tensors(self, variants, out=None):
        """pdlp_mi355x_batch_run_device: run() with every array of every variant a float64 tensor on the batch's device —
        rows of a contiguous [K, n] tensor are valid entries (tensors.stacked) — and the solutions left there.  -> one
        tensors.TensorResult per variant, bit for bit what run() gives for the same arrays as numpy.  out: None (fresh
        tensors), a list with one dict per variant as DeviceSolver.run_tensors takes it (a vector mapped to None is not
        asked for), or ONE dict of two-dimensional tensors, col_value / col_dual as [K, num_col], row_value / row_dual as
        [K, num_row], row k being variant k's vector.  The variants' tensors are read behind torch's current stream,
        without synchronising it; with `out`, that stream is synchronised first, as for DeviceSolver.run_tensors."""
        import torch

        from . import tensors as T

        K = len(variants)
        n0, m = self.lp.num_col, self.lp.num_row
        dev = torch.device("cuda", self.params.device)
        V, keep = self._tensor_variants(variants)
        if out is None:
            outs = [None] * K
        elif isinstance(out, dict):
            sizes = dict(col_value=n0, col_dual=n0, row_value=m, row_dual=m)
            unknown = set(out) - set(sizes)
            if unknown:
                raise ValueError(f"out: unknown vectors {sorted(unknown)}; the four are {T.TensorResult.VECTORS}")
            for name, t in out.items():
                if not isinstance(t, torch.Tensor):
                    raise TypeError(f"out[{name!r}]: a torch tensor is needed, got {type(t).__name__}")
                if t.dim() != 2 or tuple(t.shape) != (K, sizes[name]):
                    raise ValueError(f"out[{name!r}]: shape ({K}, {sizes[name]}) is needed, got {tuple(t.shape)}")
            outs = [{name: t[k] for name, t in out.items()} for k in range(K)]
        else:
            outs = list(out)
            if len(outs) != K:
                raise ValueError(f"out: one entry per variant is needed ({K}), got {len(outs)}")
        results = []
        Rs = (abi.PdlpResult * max(K, 1))()
        for k in range(K):
            o = outs[k] or {}
            try:
                R = T.TensorResult(n0, m, dev, {a: t for a, t in o.items() if t is not None}, [a for a, t in o.items() if t is None])
            except (TypeError, ValueError) as e:
                raise type(e)(f"variant {k}: {e}") from None
            results.append(R)
            Rs[k] = R.struct
        with torch.cuda.device(dev):
            cur = torch.cuda.current_stream()
            if out is not None:  # (what torch has queued that still reads the given tensors ends first)
                cur.synchronize()
            rc = lib().pdlp_mi355x_batch_run_device(self.h, K, V, Rs, C.c_void_p(cur.cuda_stream))
        _check(rc, "pdlp_mi355x_batch_run_device")
        del keep
        for k in range(K):
            results[k].struct = Rs[k]
        return results

    def info(self):
        """About the last run."""
        I = abi.PdlpBatchInfo()
        _check(lib().pdlp_mi355x_batch_info(self.h, C.byref(I)), "pdlp_mi355x_batch_info")
        return I

    def close(self):
        if self.h:
            lib().pdlp_mi355x_batch_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def solve_many(lps, lanes=8, starts=None, **options):
    """pdlp_mi355x_solve_many: the LPs of `lps` (HighsLp; the same object may appear more than once) solved with one set of
    options on `lanes` (1..8) lanes — where an LP's trial loop runs XCD-local, up to eight of them at once, one per XCD.
    starts: None, or one entry per LP (None, or a dict with col_value, row_value, row_dual as solveLpCupdlp takes it).
    -> (list of PdlpOutcome, one per LP and bit for bit what solveLpCupdlp(lp, start, **options) gives; abi.PdlpPoolInfo).
    Each outcome's info["pool_path"] is its abi.POOL_*.  Raises RuntimeError with the library's words when the call is
    refused or a problem fails."""
    params = options.pop("params", None) or abi.default_params(**options)
    lps = list(lps)
    K = len(lps)
    starts = [None] * K if starts is None else list(starts)
    if len(starts) != K:
        raise ValueError("starts: one entry per LP")
    handles = [abi.ProblemHandle(lp, st) for lp, st in zip(lps, starts)]
    if any(h.wide for h in handles):
        raise ValueError("pools take 32-bit column starts")
    pP = C.POINTER(abi.PdlpProblem)
    Ps = (pP * max(K, 1))()
    Rs = (abi.PdlpResult * max(K, 1))()
    results = []
    for k, (lp, h) in enumerate(zip(lps, handles)):
        Ps[k] = C.pointer(h.struct)
        R = abi.ResultHandle(lp.num_col, lp.num_row)
        results.append(R)
        Rs[k] = R.struct
    path = np.zeros(max(K, 1), dtype=np.int32)
    I = abi.PdlpPoolInfo()
    _check(lib().pdlp_mi355x_solve_many(K, Ps, C.byref(params), int(lanes), Rs, path.ctypes.data_as(abi.c_i32p), C.byref(I)),
           "pdlp_mi355x_solve_many")
    out = []
    for k in range(K):
        results[k].struct = Rs[k]
        o = _outcome(lps[k], results[k], params, 0)
        o.info["pool_path"] = int(path[k])
        out.append(o)
    return out, I


class SyntheticProblem:
    """The synthetic LP of SURVEY §8d, generated by the library (C++ std::mt19937_64)."""

    def __init__(self, m, n, nnz, seed=1):
        self.struct = abi.PdlpProblem()
        rc = lib().pdlp_mi355x_gen_synthetic(m, n, nnz, seed, C.byref(self.struct))
        if rc != 0:
            raise RuntimeError("gen_synthetic failed")

    def to_lp(self):
        P = self.struct
        n, m, nnz = P.num_col, P.num_row, P.num_nz
        g = lambda p, k: np.ctypeslib.as_array(p, shape=(k,)).copy()
        return HighsLp(n, m, g(P.col_cost, n), g(P.col_lower, n), g(P.col_upper, n), g(P.row_lower, m), g(P.row_upper, m),
                       g(P.a_start, n + 1), g(P.a_index, nnz), g(P.a_value, nnz), int(P.sense), float(P.offset),
                       "synthetic").normalise()

    def close(self):
        if self.struct.a_start:
            lib().pdlp_mi355x_free_problem(C.byref(self.struct))

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def host_prepare_qp(lp, a_value=None, q_value=None, update=None, update_then=None, params=None, **options):
    """pdlp_mi355x_host_prepare_qp: the host twin of a Hessian-updatable create (a_value, q_value and update all None) and
    of pdlp_mi355x_update_values.  update / update_then: abi.UpdateHandle or None (update_then: a pdlp_mi355x_update
    applied afterwards on the same form).  Returns (form, hessian): two dicts with every field of pdlp_prepared_t and
    pdlp_prepared_hessian_t as numpy copies / numbers."""
    params = params or abi.default_params(**options)
    keep = abi.ProblemHandle(lp)
    F, Q = abi.PdlpPrepared(), abi.PdlpPreparedHessian()
    a = None if a_value is None else np.ascontiguousarray(a_value, dtype=np.float64)
    q = None if q_value is None else np.ascontiguousarray(q_value, dtype=np.float64)
    _check(lib().pdlp_mi355x_host_prepare_qp_then(
        C.byref(keep.struct), C.byref(params), None if a is None else a.ctypes.data_as(abi.c_f64p),
        None if q is None else q.ctypes.data_as(abi.c_f64p), None if update is None else C.byref(update.struct),
        None if update_then is None else C.byref(update_then.struct), C.byref(F), C.byref(Q)), "host_prepare_qp")
    g = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt).copy() if p else np.zeros(0, dtype=dt)
    n, m, nnz = F.n, F.m, F.nnz
    form = dict(
        n=n, m=m, n_eqs=F.n_eqs, n_orig=F.n_orig, nnz=nnz,
        csr_beg=g(F.csr_beg, m + 1, np.int32), csr_idx=g(F.csr_idx, nnz, np.int32), csr_val=g(F.csr_val, nnz, np.float64),
        csc_beg=g(F.csc_beg, n + 1, np.int32), csc_idx=g(F.csc_idx, nnz, np.int32), csc_val=g(F.csc_val, nnz, np.float64),
        cost=g(F.cost, n, np.float64), rhs=g(F.rhs, m, np.float64), lower=g(F.lower, n, np.float64), upper=g(F.upper, n, np.float64),
        col_scale=g(F.col_scale, n, np.float64), row_scale=g(F.row_scale, m, np.float64),
        row_kind=g(F.row_kind, m, np.int32), row_new_idx=g(F.row_new_idx, m, np.int32),
        norm_cost=F.norm_cost, norm_rhs=F.norm_rhs, mat_norm_inf=F.mat_norm_inf,
        spmv_blocks_ax=F.spmv_blocks_ax, spmv_blocks_aty=F.spmv_blocks_aty)
    no = Q.nnz_off
    hess = dict(n=Q.n, has_diag=Q.has_diag, nnz_off=no, qdiag=g(Q.qdiag, Q.n if Q.has_diag else 0, np.float64),
                q_beg=g(Q.q_beg, Q.n + 1 if no else 0, np.int32), q_idx=g(Q.q_idx, no, np.int32), q_val=g(Q.q_val, no, np.float64))
    lib().pdlp_mi355x_free_prepared(C.byref(F))
    lib().pdlp_mi355x_free_prepared_hessian(C.byref(Q))
    return form, hess


# reason codes of the rule that decides where a QP's Hessian is extracted (csrc/pdlp_setup.hpp hessianExtractionReason)
HESSIAN_REASONS = ("on_device", "host_setup", "sharded", "hipdlp", "no_slots", "q_start", "switched_off")


def hessian_extraction_rule(q_start, gpu_setup=True, sharded=False, hipdlp=False, switch_on=True):
    """pdlp_mi355x_host_hessian_extraction_rule (a test hook outside the public header; needs no device): the name of the
    rule's reason for a Hessian with these column starts (None: no Hessian)."""
    fn = lib().pdlp_mi355x_host_hessian_extraction_rule
    fn.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, abi.c_i32p, C.POINTER(C.c_int32)]
    st = None if q_start is None else np.ascontiguousarray(q_start, dtype=np.int32)
    reason = C.c_int32(-1)
    _check(fn(int(gpu_setup), int(sharded), int(hipdlp), int(switch_on), 0 if st is None else len(st) - 1,
              None if st is None else st.ctypes.data_as(abi.c_i32p), C.byref(reason)), "hessian_extraction_rule")
    return HESSIAN_REASONS[reason.value]


def stream_plan(form, which, slab_long_limit=0, extra_blocks=0):
    """pdlp_mi355x_host_stream_plan: the work plan of operand `which` (0: A by rows, 1: A' by columns) of a prepared form
    as the device set-up builds it.  form: a Prepared, or a dict with n, m, nnz, csr_beg / csr_idx / csr_val, csc_beg / csc_idx /
    csc_val, spmv_blocks_ax, spmv_blocks_aty (the first dict of host_prepare_qp).  slab_long_limit = 0: the stream layout —
    blocks [n_blocks, 4] (first major, end major, first entry, end entry), long_majors, tasks [n_tasks, 8] (pdlp_task_plan_t's
    records; column 2 is -1 for an idle task); > 0: the slab layout's long majors only.  long_group: long majors per
    contribution slot; small_grid: workgroups of the persistent trial loop where the operands qualify (extra_blocks: work blocks
    of a third operand)."""
    get = (lambda k: form[k]) if isinstance(form, dict) else (lambda k: getattr(form, k))
    F = abi.PdlpPrepared()
    F.n, F.m, F.nnz = int(get("n")), int(get("m")), int(get("nnz"))
    F.spmv_blocks_ax, F.spmv_blocks_aty = int(get("spmv_blocks_ax")), int(get("spmv_blocks_aty"))
    keep = {}
    for k, dt, ty in (("csr_beg", np.int32, abi.c_i32p), ("csr_idx", np.int32, abi.c_i32p), ("csr_val", np.float64, abi.c_f64p),
                      ("csc_beg", np.int32, abi.c_i32p), ("csc_idx", np.int32, abi.c_i32p), ("csc_val", np.float64, abi.c_f64p)):
        keep[k] = np.ascontiguousarray(get(k), dtype=dt)
        setattr(F, k, keep[k].ctypes.data_as(ty))
    SP = abi.PdlpStreamPlan()
    _check(lib().pdlp_mi355x_host_stream_plan(C.byref(F), which, slab_long_limit, extra_blocks, C.byref(SP)), "stream_plan")
    g = lambda p, k: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(np.int64).copy() if p else np.zeros(0, np.int64)
    out = dict(chunk=SP.chunk, n_blocks=SP.n_blocks, n_long=SP.n_long, n_tasks=SP.n_tasks, task_group=SP.task_group,
               long_group=SP.long_group, long_slots=SP.long_slots, small_grid=SP.small_grid,
               blocks=g(SP.block_beg, 4 * SP.n_blocks).reshape(-1, 4), long_majors=g(SP.long_majors, SP.n_long),
               tasks=g(SP.tasks, 8 * SP.n_tasks).reshape(-1, 8))
    lib().pdlp_mi355x_free_stream_plan(C.byref(SP))
    return out


class Prepared:
    """Host-side standard form built by the PRODUCT library (pdlp_mi355x_host_prepare); numpy copies."""

    def __init__(self, lp=None, params=None, problem_struct=None, slab_long_limit=256, update=None, update_matrix=None, **options):
        """update: an abi.UpdateHandle — the form then comes from pdlp_mi355x_host_prepare_updated (the host twin of
        pdlp_mi355x_update: prepare, keep the scaling passes, replay the update).
        update_matrix: (a_value, abi.UpdateHandle or None) — the form comes from pdlp_mi355x_host_prepare_updated_matrix,
        the host twin of pdlp_mi355x_update_matrix; with `update` as well, that update follows it on the same form."""
        params = params or abi.default_params(**options)
        keep = None
        if problem_struct is None:
            keep = abi.ProblemHandle(lp)
            problem_struct = keep.struct
        F = abi.PdlpPrepared()
        if update_matrix is not None:
            a, um = update_matrix
            a = None if a is None else np.ascontiguousarray(a, dtype=np.float64)
            _check(lib().pdlp_mi355x_host_prepare_updated_matrix_then(
                C.byref(problem_struct), C.byref(params), None if a is None else a.ctypes.data_as(abi.c_f64p),
                None if um is None else C.byref(um.struct), None if update is None else C.byref(update.struct), C.byref(F)),
                "host_prepare_updated_matrix")
        elif update is None:
            _check(lib().pdlp_mi355x_host_prepare(C.byref(problem_struct), C.byref(params), C.byref(F)), "host_prepare")
        else:
            _check(lib().pdlp_mi355x_host_prepare_updated(C.byref(problem_struct), C.byref(params), C.byref(update.struct), C.byref(F)),
                   "host_prepare_updated")
        n, m, nnz = F.n, F.m, F.nnz
        self.n, self.m, self.n_eqs, self.n_orig, self.nnz = n, m, F.n_eqs, F.n_orig, nnz
        g = lambda p, k, dt: np.ctypeslib.as_array(p, shape=(max(k, 1),))[:k].astype(dt).copy()
        self.csr_beg = g(F.csr_beg, m + 1, np.int32); self.csr_idx = g(F.csr_idx, nnz, np.int32); self.csr_val = g(F.csr_val, nnz, np.float64)
        self.csc_beg = g(F.csc_beg, n + 1, np.int32); self.csc_idx = g(F.csc_idx, nnz, np.int32); self.csc_val = g(F.csc_val, nnz, np.float64)
        self.cost = g(F.cost, n, np.float64); self.rhs = g(F.rhs, m, np.float64)
        self.lower = g(F.lower, n, np.float64); self.upper = g(F.upper, n, np.float64)
        self.col_scale = g(F.col_scale, n, np.float64); self.row_scale = g(F.row_scale, m, np.float64)
        self.row_kind = g(F.row_kind, m, np.int32); self.row_new_idx = g(F.row_new_idx, m, np.int32)
        self.norm_cost, self.norm_rhs, self.mat_norm_inf = F.norm_cost, F.norm_rhs, F.mat_norm_inf
        self.spmv_blocks_ax, self.spmv_blocks_aty = F.spmv_blocks_ax, F.spmv_blocks_aty
        self._slabs = {}
        for which in (0, 1):
            SL = abi.PdlpSlabLayout()
            _check(lib().pdlp_mi355x_host_slab_layout(C.byref(F), which, slab_long_limit, C.byref(SL)), "slab_layout")
            nb, R = SL.n_blocks, SL.rows_per_block
            self._slabs[which] = dict(
                rows_per_block=R, n_blocks=nb, minor_bits=SL.minor_bits, wave_beg=g(SL.wave_beg, 16 * nb + 1, np.int64),
                slab_width_log2=SL.slab_width_log2, wave_ptr=g(SL.wave_ptr, 16 * nb + 1, np.int64),
                ent=g(SL.ent, SL.nnz_short, np.uint32), val=g(SL.val, SL.nnz_short, np.float64),
                long_mask=g(SL.long_mask, (n if which else m) // 32 + 1, np.uint32), long_map=g(SL.long_map, SL.n_long, np.int32))
            lib().pdlp_mi355x_free_slab_layout(C.byref(SL))
        self._tasks = {}
        for which in (0, 1):
            for balance in (0, 1):
                TP = abi.PdlpTaskPlan()
                _check(lib().pdlp_mi355x_host_task_plan(C.byref(F), which, slab_long_limit, balance, C.byref(TP)), "task_plan")
                nl = TP.n_long
                lb = g(TP.long_beg, nl + 1, np.int64)
                self._tasks[which, balance] = dict(
                    n_tasks=TP.n_tasks, task_group=TP.task_group, n_seg_slots=TP.n_seg_slots, n_long=nl, n_blocks=TP.n_blocks,
                    tile_log2=TP.tile_log2, tasks=g(TP.tasks, 8 * TP.n_tasks, np.int64).reshape(-1, 8),
                    tile_owner=g(TP.tile_owner, TP.n_tiles, np.int64), long_beg=lb, long_idx=g(TP.long_idx, int(lb[-1]) if nl else 0, np.int64))
                lib().pdlp_mi355x_free_task_plan(C.byref(TP))
        self._parts = {}
        for w in (1, 2, 3, 4, 8):
            off = np.zeros(w + 1, dtype=np.int32)
            _check(lib().pdlp_mi355x_row_partition(C.byref(F), w, off.ctypes.data_as(abi.c_i32p)), "row_partition")
            self._parts[w] = off
        lib().pdlp_mi355x_free_prepared(C.byref(F))

    def row_partition(self, world):
        return self._parts[world]

    def task_plan(self, which, balance=1):
        """Segment tasks of the long majors of operand `which` as the slab launches run them (pdlp_task_plan_t)."""
        return self._tasks[which, balance]

    def slab_layout(self, which):
        """which = 0: A by rows, 1: A' by columns."""
        return self._slabs[which]
