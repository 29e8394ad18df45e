"""ctypes mirror of include/pdlp_mi355x.h (the C-ABI drop-in boundary).

Only plain C types cross the boundary: int32/int64/double and pointers to
caller-owned numpy buffers.  Field order and types must match the header
exactly; tests/test_host.py::test_struct_sizes_match_ctypes_mirror checks the struct sizes against the library.
"""
import ctypes as C

import numpy as np

c_i32p = C.POINTER(C.c_int32)
c_i64p = C.POINTER(C.c_int64)
INT32_MAX = 2**31 - 1
c_f64p = C.POINTER(C.c_double)

# termination codes, cuPDLP-C termination_code (cupdlp_defs.h:61-68)
TERM_OPTIMAL = 0
TERM_INFEASIBLE = 1
TERM_UNBOUNDED = 2
TERM_INFEASIBLE_OR_UNBOUNDED = 3
TERM_TIMELIMIT_OR_ITERLIMIT = 4
TERM_FEASIBLE = 5

# pdlp_features_off bits, HConst.h:417-422
FEATURE_SCALING_OFF = 1
FEATURE_RESTART_OFF = 2
FEATURE_ADAPTIVE_STEP_OFF = 4


class PdlpProblem(C.Structure):
    _fields_ = [
        ("num_col", C.c_int32),
        ("num_row", C.c_int32),
        ("num_nz", C.c_int64),
        ("a_start", c_i32p),
        ("a_index", c_i32p),
        ("a_value", c_f64p),
        ("col_cost", c_f64p),
        ("col_lower", c_f64p),
        ("col_upper", c_f64p),
        ("row_lower", c_f64p),
        ("row_upper", c_f64p),
        ("offset", C.c_double),
        ("sense", C.c_int32),
        ("start_col_value", c_f64p),
        ("start_row_value", c_f64p),
        ("start_row_dual", c_f64p),
        ("start_value_valid", C.c_int32),
        ("start_dual_valid", C.c_int32),
        ("q_dim", C.c_int32),          # HighsHessian (lower-triangular CSC); only diagonal Q is solved
        ("reserved_q", C.c_int32),
        ("q_start", c_i32p),
        ("q_index", c_i32p),
        ("q_value", c_f64p),
    ]


class PdlpParams(C.Structure):
    _fields_ = [
        ("primal_tol", C.c_double),
        ("dual_tol", C.c_double),
        ("gap_tol", C.c_double),
        ("time_limit", C.c_double),
        ("iter_limit", C.c_int32),
        ("features_off", C.c_int32),
        ("restart_method", C.c_int32),
        ("log_level", C.c_int32),
        ("device", C.c_int32),
        ("check_interval", C.c_int32),
        ("reserved", C.c_int32 * 2),
        ("algorithm", C.c_int32),           # 0 = cuPDLP-C path, 1 = HiPDLP (solver="hipdlp")
        ("scaling_mode", C.c_int32),        # pdlp_scaling_mode: 1 Ruiz | 2 L2 | 4 PC
        ("ruiz_iterations", C.c_int32),     # pdlp_ruiz_iterations
        ("step_size_strategy", C.c_int32),  # pdlp_step_size_strategy: 0 fixed, else PID
        ("num_devices", C.c_int32),         # pdlp_mi355x_solve: shard over this many devices of the process
        ("updatable", C.c_int32),           # create: keep what pdlp_mi355x_update replays (per-pass scale factors, row kinds)
        ("log_callback", C.c_void_p),       # void (*)(void* ctx, int level, const char* text); NULL = stdout
        ("log_ctx", C.c_void_p),
    ]


class PdlpResult(C.Structure):
    _fields_ = [
        ("col_value", c_f64p),
        ("col_dual", c_f64p),
        ("row_value", c_f64p),
        ("row_dual", c_f64p),
        ("value_valid", C.c_int32),
        ("dual_valid", C.c_int32),
        ("term_code", C.c_int32),
        ("term_iterate", C.c_int32),
        ("num_iter", C.c_int32),
        ("num_trials", C.c_int32),
        ("num_restarts", C.c_int32),
        ("reserved_i", C.c_int32),
        ("primal_obj", C.c_double),
        ("dual_obj", C.c_double),
        ("primal_feas", C.c_double),
        ("dual_feas", C.c_double),
        ("rel_gap", C.c_double),
        ("norm_rhs", C.c_double),
        ("norm_cost", C.c_double),
        ("setup_seconds", C.c_double),
        ("solve_seconds", C.c_double),
        ("reserved_d", C.c_double * 4),
    ]


UPDATABLE_DATA, UPDATABLE_MATRIX = 1, 2  # pdlp_params_t.updatable bits
UPDATABLE_HESSIAN = 4                    # implies DATA, independent of MATRIX


class PdlpUpdate(C.Structure):
    """pdlp_update_t (include/pdlp_mi355x.h): new data for a held solver; NULL = unchanged."""
    _fields_ = [
        ("col_cost", c_f64p),
        ("col_lower", c_f64p),
        ("col_upper", c_f64p),
        ("row_lower", c_f64p),
        ("row_upper", c_f64p),
        ("offset", C.c_double),
        ("has_offset", C.c_int32),
        ("reserved", C.c_int32),
        ("start_col_value", c_f64p),
        ("start_row_value", c_f64p),
        ("start_row_dual", c_f64p),
    ]


class PdlpVariant(C.Structure):
    """pdlp_variant_t (include/pdlp_mi355x.h): one variant of pdlp_mi355x_batch_run_values; its size is checked against
    pdlp_mi355x_variant_size()."""
    _fields_ = [
        ("a_value", c_f64p),
        ("num_nz", C.c_int64),
        ("q_value", c_f64p),
        ("num_q_nz", C.c_int64),
        ("u", PdlpUpdate),
    ]


# The keys of one variant of DeviceBatch.run / run_tensors: PdlpVariant's arrays, PdlpUpdate's, and the variant's own limit
VARIANT_KEYS = ("a_value", "q_value", "col_cost", "col_lower", "col_upper", "row_lower", "row_upper", "offset", "start", "iter_limit")


# pdlp_session_info_t.path / .changed (include/pdlp_mi355x.h)
SESSION_NONE, SESSION_CREATE, SESSION_UPDATE, SESSION_UPDATE_MATRIX, SESSION_UPDATE_VALUES, SESSION_ONE_SHOT = range(6)
SESSION_PATH_NAME = {0: "none", 1: "create", 2: "update", 3: "update matrix", 4: "update values", 5: "one-shot"}
CHANGED_PATTERN, CHANGED_MATRIX_VALUES, CHANGED_HESSIAN_PATTERN, CHANGED_HESSIAN_VALUES = 1, 2, 4, 8
CHANGED_COST, CHANGED_COL_LOWER, CHANGED_COL_UPPER, CHANGED_ROW_BOUNDS, CHANGED_OFFSET = 16, 32, 64, 128, 256
CHANGED_RUNTIME_OPTIONS, CHANGED_STRUCTURAL_OPTIONS, CHANGED_SHAPE = 512, 1024, 2048


class PdlpSessionInfo(C.Structure):
    """pdlp_session_info_t (include/pdlp_mi355x.h): what the last pdlp_mi355x_session_solve found and did; its size is
    checked against pdlp_mi355x_session_info_size()."""
    _fields_ = [
        ("path", C.c_int32),
        ("changed", C.c_int32),
        ("kind_row", C.c_int32),
        ("kind_was", C.c_int32),
        ("kind_now", C.c_int32),
        ("reserved", C.c_int32),
        ("diff_seconds", C.c_double),
        ("upload_seconds", C.c_double),
        ("apply_seconds", C.c_double),
        ("setup_seconds", C.c_double),
        ("held_bytes", C.c_int64),
        ("reason", C.c_char * 160),
    ]

    @property
    def text(self):
        return self.reason.decode()


class PdlpBatchInfo(C.Structure):
    """pdlp_batch_info_t (include/pdlp_mi355x.h): what the last pdlp_mi355x_batch_run did; its size is checked against
    pdlp_mi355x_batch_info_size()."""
    _fields_ = [
        ("lanes", C.c_int32),
        ("lanes_concurrent", C.c_int32),
        ("variants", C.c_int32),
        ("trial_launches", C.c_int32),
        ("check_launches", C.c_int32),
        ("fallback_variants", C.c_int32),
        ("xcc_of_lane", C.c_int32 * 8),
        ("reserved", C.c_int32 * 2),
        ("wall_seconds", C.c_double),
        ("reason", C.c_char * 160),
    ]

    @property
    def text(self):
        return self.reason.decode()


# pdlp_mi355x_solve_many: path[k] (include/pdlp_mi355x.h)
POOL_NOT_RUN, POOL_SHARED, POOL_ALONE, POOL_FALLBACK = range(4)


class PdlpPoolInfo(C.Structure):
    """pdlp_pool_info_t (include/pdlp_mi355x.h): what a pdlp_mi355x_solve_many did; its size is checked against
    pdlp_mi355x_pool_info_size()."""
    _fields_ = [
        ("problems", C.c_int32),
        ("lanes", C.c_int32),
        ("lanes_concurrent", C.c_int32),
        ("shared_problems", C.c_int32),
        ("alone_problems", C.c_int32),
        ("fallback_problems", C.c_int32),
        ("trial_launches", C.c_int32),
        ("check_launches", C.c_int32),
        ("mixed_launches", C.c_int32),
        ("xcc_of_lane", C.c_int32 * 8),
        ("reserved", C.c_int32 * 3),
        ("wall_seconds", C.c_double),
        ("create_seconds", C.c_double),
        ("reason", C.c_char * 160),
    ]

    @property
    def text(self):
        return self.reason.decode()


class PdlpIterStats(C.Structure):
    _fields_ = [
        ("iters", C.c_int32),
        ("trials", C.c_int32),
        ("checks", C.c_int32),
        ("restarts", C.c_int32),
        ("gpu_ms", C.c_double),
        ("wall_ms", C.c_double),
        ("spmv_ax_ms", C.c_double),
        ("spmv_aty_ms", C.c_double),
        ("reserved", C.c_double * 4),
    ]


class PdlpPrepared(C.Structure):
    _fields_ = [
        ("n", C.c_int32), ("m", C.c_int32), ("n_eqs", C.c_int32), ("n_orig", C.c_int32),
        ("nnz", C.c_int64),
        ("csr_beg", c_i32p), ("csr_idx", c_i32p), ("csr_val", c_f64p),
        ("csc_beg", c_i32p), ("csc_idx", c_i32p), ("csc_val", c_f64p),
        ("cost", c_f64p), ("rhs", c_f64p), ("lower", c_f64p), ("upper", c_f64p),
        ("col_scale", c_f64p), ("row_scale", c_f64p),
        ("row_kind", c_i32p), ("row_new_idx", c_i32p),
        ("norm_cost", C.c_double), ("norm_rhs", C.c_double), ("mat_norm_inf", C.c_double),
        ("spmv_blocks_ax", C.c_int32), ("spmv_blocks_aty", C.c_int32),
    ]


class PdlpPreparedHessian(C.Structure):
    """pdlp_prepared_hessian_t (include/pdlp_mi355x.h): the scaled Hessian of a prepared form, for the CPU tests."""
    _fields_ = [
        ("n", C.c_int32), ("has_diag", C.c_int32),
        ("nnz_off", C.c_int64),
        ("qdiag", c_f64p), ("q_beg", c_i32p), ("q_idx", c_i32p), ("q_val", c_f64p),
    ]


class PdlpSlabLayout(C.Structure):
    _fields_ = [
        ("rows_per_block", C.c_int32), ("rows_per_wave", C.c_int32), ("n_blocks", C.c_int32), ("minor_bits", C.c_int32),
        ("slab_width_log2", C.c_int32), ("n_long", C.c_int32),
        ("nnz_short", C.c_int64),
        ("wave_ptr", c_i32p), ("ent", C.POINTER(C.c_uint32)), ("val", c_f64p),
        ("long_mask", C.POINTER(C.c_uint32)), ("long_map", c_i32p), ("wave_beg", c_i32p),
    ]


class PdlpTaskPlan(C.Structure):
    """pdlp_task_plan_t (include/pdlp_mi355x.h): the segment tasks of a slab operand's long majors, for the CPU tests."""
    _fields_ = [
        ("n_tasks", C.c_int32), ("task_group", C.c_int32), ("n_seg_slots", C.c_int32), ("n_long", C.c_int32),
        ("n_blocks", C.c_int32), ("tile_log2", C.c_int32), ("n_tiles", C.c_int32), ("reserved", C.c_int32),
        ("tasks", c_i32p), ("tile_owner", C.POINTER(C.c_int8)), ("long_beg", c_i32p), ("long_idx", c_i32p),
    ]


class PdlpStreamPlan(C.Structure):
    """pdlp_stream_plan_t (csrc/pdlp_api.cpp, a test hook outside the public header): the work plan of a stream-layout
    operand, for the CPU tests."""
    _fields_ = [
        ("chunk", C.c_int32), ("n_blocks", C.c_int32), ("n_long", C.c_int32), ("n_tasks", C.c_int32),
        ("task_group", C.c_int32), ("long_group", C.c_int32), ("long_slots", C.c_int32), ("small_grid", C.c_int32),
        ("block_beg", c_i32p), ("long_majors", c_i32p), ("tasks", c_i32p),
    ]


class PdlpDeviceMatrix(C.Structure):
    """pdlp_device_matrix_t (csrc/pdlp_api.cpp, a test hook outside the public header): what a solver holds of one
    operand after its set-up, for the GPU tests of the device-side set-up."""
    _fields_ = [
        ("use_slab", C.c_int32), ("n_major", C.c_int32), ("n_minor", C.c_int32), ("chunk", C.c_int32),
        ("n_blocks", C.c_int32), ("slab_blocks", C.c_int32), ("rows_per_block", C.c_int32), ("minor_bits", C.c_int32),
        ("slab_width_log2", C.c_int32), ("n_long", C.c_int32), ("n_tasks", C.c_int32), ("task_group", C.c_int32),
        ("long_group", C.c_int32), ("long_slots", C.c_int32), ("tile_log2", C.c_int32), ("n_tiles", C.c_int32),
        ("n_mask_words", C.c_int32), ("n_csr_major", C.c_int32),
        ("nnz", C.c_int64), ("nnz_short", C.c_int64), ("nnz_csr", C.c_int64),
        ("beg", c_i32p), ("idx", c_i32p), ("block_beg", c_i32p), ("wave_beg", c_i32p), ("wave_ptr", c_i32p),
        ("long_map", c_i32p), ("tasks", c_i32p), ("span_lo", c_i32p), ("span_hi", c_i32p), ("span_cnt", c_i32p),
        ("ent", C.POINTER(C.c_uint32)), ("long_mask", C.POINTER(C.c_uint32)),
        ("val", c_f64p), ("slab_val", c_f64p),
        ("tile_owner", C.POINTER(C.c_int8)),
    ]


class PdlpMpsModel(C.Structure):
    """pdlp_mps_model_t (include/pdlp_mi355x.h): what pdlp_mi355x_read_mps fills."""
    _fields_ = [
        ("lp", PdlpProblem),
        ("cost_row_location", C.c_int32), ("num_integrality", C.c_int32),
        ("integrality", C.POINTER(C.c_uint8)),
        ("model_name", C.c_char_p), ("objective_name", C.c_char_p),
        ("col_name_pool", C.POINTER(C.c_char)), ("col_name_start", C.POINTER(C.c_int64)),
        ("row_name_pool", C.POINTER(C.c_char)), ("row_name_start", C.POINTER(C.c_int64)),
        ("hessian_dim", C.c_int32), ("warning_issued", C.c_int32),
        ("hessian_start", c_i32p), ("hessian_index", c_i32p), ("hessian_value", c_f64p),
        ("num_warnings", C.c_int32), ("threads", C.c_int32),
        ("warnings", C.c_char_p),
        ("file_bytes", C.c_int64), ("seconds", C.c_double),
    ]


def default_params(**kw):
    """Defaults HiGHS passes for default options (CupdlpWrapper.cpp:642-717;
    kkt_tolerance default 1e-7, HConst.h:345)."""
    p = PdlpParams()
    p.primal_tol = 1e-7
    p.dual_tol = 1e-7
    p.gap_tol = 1e-7
    p.time_limit = float("inf")
    p.iter_limit = 2**31 - 1
    p.features_off = 0
    p.restart_method = 1
    p.log_level = 0
    p.device = 0
    p.check_interval = 0
    p.algorithm = 0
    p.scaling_mode = 5          # kPdlpScalingRuiz + kPdlpScalingPC, HighsOptions.h:1345-1349
    p.ruiz_iterations = 10      # HighsOptions.h:1353-1355
    p.step_size_strategy = 1    # kPdlpStepSizeStrategyAdaptive, HighsOptions.h:1374-1378 (HiPDLP: -> PID)
    for k, v in kw.items():
        if k == "kkt_tolerance":
            p.primal_tol = p.dual_tol = p.gap_tol = float(v)
        elif k == "pdlp_iteration_limit":
            p.iter_limit = int(min(v, 2**31 - 1))
        elif k == "pdlp_features_off":
            p.features_off = int(v)
        elif k == "solver":
            p.algorithm = {"pdlp": 0, "hipdlp": 1}[v]
        elif k in ("pdlp_scaling_mode", "pdlp_ruiz_iterations", "pdlp_step_size_strategy"):
            setattr(p, k[5:], int(v))
        elif k == "updatable":
            # "matrix", or an int with UPDATABLE_MATRIX set: PDLP_UPDATABLE_DATA | PDLP_UPDATABLE_MATRIX (pdlp_mi355x_update_matrix
            # too); "hessian" / "matrix+hessian", or an int with UPDATABLE_HESSIAN set: PDLP_UPDATABLE_HESSIAN as well
            # (pdlp_mi355x_update_values); any other truthy value: DATA
            if isinstance(v, str):
                parts = v.split("+")
                matrix, hessian = "matrix" in parts, "hessian" in parts
            else:
                is_mask = not isinstance(v, bool) and isinstance(v, int)
                matrix, hessian = bool(is_mask and v & UPDATABLE_MATRIX), bool(is_mask and v & UPDATABLE_HESSIAN)
            p.updatable = ((UPDATABLE_MATRIX if matrix else 0) | (UPDATABLE_HESSIAN if hessian else 0) |
                           (UPDATABLE_DATA if (v or matrix or hessian) else 0))
        elif k == "device_reduction_order":
            # ORACLE ONLY: sum the reductions in the HIP kernels' order (oracle/pdlp_oracle.c, GPU-ORDER)
            p.reserved[0] = 1 if v else 0
        elif k == "device_layout":
            # ORACLE ONLY: which SpMV work plan to restate: "auto" (the product's rule), "csr", "slab"
            p.reserved[1] = {"auto": 0, "csr": 1, "slab": 2}[v]
        else:
            setattr(p, k, v)
    return p


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _ptr(a, ty):
    return a.ctypes.data_as(ty)


class ProblemHandle:
    """Owns the numpy buffers a pdlp_problem_t points to.  Column starts above INT32_MAX (an int64 array) stay 64-bit:
    `wide` is set, struct.a_start is NULL and `a_start` is the array the *_wide entries take instead."""

    def __init__(self, lp, start=None):
        self.lp = lp
        st = np.asarray(lp.a_start)
        self.wide = st.size > 0 and int(st.max()) > INT32_MAX
        self.a_start = np.ascontiguousarray(st, dtype=np.int64) if self.wide else _i32(st)
        self.a_index = _i32(lp.a_index)
        self.a_value = _f64(lp.a_value)
        self.col_cost = _f64(lp.col_cost)
        self.col_lower = _f64(lp.col_lower)
        self.col_upper = _f64(lp.col_upper)
        self.row_lower = _f64(lp.row_lower)
        self.row_upper = _f64(lp.row_upper)
        P = PdlpProblem()
        P.num_col = int(lp.num_col)
        P.num_row = int(lp.num_row)
        P.num_nz = int(self.a_start[lp.num_col])
        P.a_start = None if self.wide else _ptr(self.a_start, c_i32p)
        P.a_index = _ptr(self.a_index, c_i32p)
        P.a_value = _ptr(self.a_value, c_f64p)
        P.col_cost = _ptr(self.col_cost, c_f64p)
        P.col_lower = _ptr(self.col_lower, c_f64p)
        P.col_upper = _ptr(self.col_upper, c_f64p)
        P.row_lower = _ptr(self.row_lower, c_f64p)
        P.row_upper = _ptr(self.row_upper, c_f64p)
        P.offset = float(lp.offset)
        P.sense = int(lp.sense)
        if start is not None:
            self.s_col = _f64(start["col_value"])
            self.s_rowv = _f64(start["row_value"])
            self.s_rowd = _f64(start["row_dual"])
            P.start_col_value = _ptr(self.s_col, c_f64p)
            P.start_row_value = _ptr(self.s_rowv, c_f64p)
            P.start_row_dual = _ptr(self.s_rowd, c_f64p)
            P.start_value_valid = 1
            P.start_dual_valid = 1
        hess = getattr(lp, "hessian", None)
        if hess is not None:  # (start, index, value) of a lower-triangular column-wise HighsHessian
            self.q_start, self.q_index, self.q_value = _i32(hess[0]), _i32(hess[1]), _f64(hess[2])
            P.q_dim = len(self.q_start) - 1
            P.q_start = _ptr(self.q_start, c_i32p)
            P.q_index = _ptr(self.q_index, c_i32p)
            P.q_value = _ptr(self.q_value, c_f64p)
        self.struct = P


class ResultHandle:
    def __init__(self, num_col, num_row):
        self.col_value = np.zeros(num_col)
        self.col_dual = np.zeros(num_col)
        self.row_value = np.zeros(max(num_row, 1))[:num_row]
        self.row_dual = np.zeros(max(num_row, 1))[:num_row]
        R = PdlpResult()
        R.col_value = _ptr(self.col_value, c_f64p)
        R.col_dual = _ptr(self.col_dual, c_f64p)
        R.row_value = _ptr(self.row_value, c_f64p)
        R.row_dual = _ptr(self.row_dual, c_f64p)
        self.struct = R

    def __getattr__(self, k):
        return getattr(self.__dict__["struct"], k)


class UpdateHandle:
    """Owns the numpy buffers a pdlp_update_t points to.  None = unchanged; `start` is a dict with col_value, row_value
    and row_dual (all three) or None for a cold start.  Partial input (one row bound, part of a start) is passed on as it
    is: the library refuses it with its own message."""

    def __init__(self, col_cost=None, col_lower=None, col_upper=None, row_lower=None, row_upper=None, offset=None, start=None):
        U = PdlpUpdate()
        self._keep = []

        def put(name, a):
            if a is None:
                return
            a = _f64(a)
            self._keep.append(a)
            setattr(U, name, _ptr(a, c_f64p))

        put("col_cost", col_cost)
        put("col_lower", col_lower)
        put("col_upper", col_upper)
        put("row_lower", row_lower)
        put("row_upper", row_upper)
        if offset is not None:
            U.offset = float(offset)
            U.has_offset = 1
        if start is not None:
            put("start_col_value", start.get("col_value"))
            put("start_row_value", start.get("row_value"))
            put("start_row_dual", start.get("row_dual"))
        self.struct = U


class VariantHandle:
    """Owns the numpy buffers a pdlp_variant_t points to: a_value / q_value (None = the values of the batch's problem) and
    the arguments of UpdateHandle."""

    def __init__(self, a_value=None, q_value=None, **update):
        self.update = UpdateHandle(**update)
        self.a_value = None if a_value is None else _f64(a_value)
        self.q_value = None if q_value is None else _f64(q_value)
        V = PdlpVariant()
        if self.a_value is not None:
            V.a_value = _ptr(self.a_value, c_f64p)
            V.num_nz = self.a_value.size
        if self.q_value is not None:
            V.q_value = _ptr(self.q_value, c_f64p)
            V.num_q_nz = self.q_value.size
        V.u = self.update.struct
        self.struct = V
