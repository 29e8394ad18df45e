/*
 * pdlp_mi355x.h — C ABI of the MI355X-native PDLP hot path for HiGHS.
 *
 * This is the drop-in boundary for ONE path of ERGO-Code/HiGHS: the PDLP
 * first-order LP solver reached through Highs::run() with solver="pdlp"
 * (and, with pdlp_params_t.algorithm = 1, its sibling solver="hipdlp":
 * highs/pdlp/HiPdlpWrapper.cpp, replaced by integration/HiPdlpWrapperMi355x.cpp).
 * The entry points below are exactly what the reference wrapper
 * (highs/pdlp/CupdlpWrapper.cpp) would bind instead of its calls into the
 * vendored cuPDLP-C:
 *
 *   reference call (file:line)                               replaced by
 *   -------------------------------------------------------  --------------------------
 *   formulateLP_highs      CupdlpWrapper.cpp:104,280-448  \
 *   Init_Scaling           CupdlpWrapper.cpp:110           |
 *   PDHG_Scale_Data        CupdlpWrapper.cpp:153           |  pdlp_mi355x_create
 *   problem_alloc          CupdlpWrapper.cpp:161,517-585   |
 *   PDHG_Alloc             CupdlpWrapper.cpp:167          /
 *   LP_SolvePDHG           CupdlpWrapper.cpp:199,
 *                          cupdlp_solver.c:1437-1498          pdlp_mi355x_run
 *   PDHG_Destroy + frees   CupdlpWrapper.cpp:218,253-269      pdlp_mi355x_destroy
 *   (all of the above, one shot)                              pdlp_mi355x_solve
 *   (create / run with every array in HBM already)            pdlp_mi355x_create_device, pdlp_mi355x_run_device
 *
 * Plain C types only: pointers, sizes, doubles, int32. No C++/torch types.
 * All input arrays are caller-owned and read-only; all output arrays are
 * caller-allocated (mirrors highs_solution.*.resize, CupdlpWrapper.cpp:190-193).
 * No function here ever calls exit()/abort() or throws across the boundary;
 * failures are reported through the return code (0 = RETCODE_OK,
 * cupdlp glbopts.h:250-256) and pdlp_mi355x_last_error().
 *
 * Arithmetic is fp64, indices are int32 (cupdlp_int / HighsInt default,
 * glbopts.h:258-263); the *_wide entries also take 64-bit column starts.
 */
#ifndef PDLP_MI355X_H_
#define PDLP_MI355X_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PDLP_MI355X_ABI_VERSION 6

/* Termination codes: same numbering as cuPDLP-C's termination_code
 * (cupdlp_defs.h:61-68) so the status map of CupdlpWrapper.cpp:225-251
 * applies unchanged. */
enum {
  PDLP_TERM_OPTIMAL = 0,
  PDLP_TERM_INFEASIBLE = 1,
  PDLP_TERM_UNBOUNDED = 2,
  PDLP_TERM_INFEASIBLE_OR_UNBOUNDED = 3,
  PDLP_TERM_TIMELIMIT_OR_ITERLIMIT = 4,
  PDLP_TERM_FEASIBLE = 5
};

/* pdlp_features_off bitmask, HConst.h:417-422 */
enum {
  PDLP_FEATURE_SCALING_OFF = 1,
  PDLP_FEATURE_RESTART_OFF = 2,
  PDLP_FEATURE_ADAPTIVE_STEP_OFF = 4
};

/* The LP exactly as HiGHS holds it in HighsLp (lp_data/HighsLp.h), column-wise:
 *   min/max  sense * (col_cost' x) + offset
 *   s.t.     row_lower <= A x <= row_upper,  col_lower <= x <= col_upper
 * Infinite bounds are +-inf or any |value| >= 1e20 (CupdlpWrapper.cpp:316-317). */
typedef struct pdlp_problem {
  int32_t num_col;
  int32_t num_row;
  int64_t num_nz;
  const int32_t* a_start; /* [num_col+1] CSC column starts   (lp.a_matrix_.start_) */
  const int32_t* a_index; /* [num_nz]    row indices         (lp.a_matrix_.index_) */
  const double* a_value;  /* [num_nz]                         (lp.a_matrix_.value_) */
  const double* col_cost; /* [num_col] */
  const double* col_lower;
  const double* col_upper;
  const double* row_lower; /* [num_row] */
  const double* row_upper;
  double offset;
  int32_t sense; /* +1 minimise, -1 maximise (ObjSense) */
  /* Optional hot start (PDHG_PreSolve, cupdlp_solver.c:1217-1279); used only
   * when BOTH value_valid and dual_valid are non-zero. May be NULL. */
  const double* start_col_value; /* [num_col] */
  const double* start_row_value; /* [num_row] */
  const double* start_row_dual;  /* [num_row] */
  int32_t start_value_valid;
  int32_t start_dual_valid;
  /* Optional quadratic objective  + 1/2 x' Q x  (no reference counterpart on the PDLP
   * path: HiGHS gates solver="pdlp" to LPs, lp_data/HighsOptions.cpp:1178-1181).  Q as HiGHS holds it in
   * HighsHessian (model/HighsHessian.h:22-34): lower-triangular, column-wise, dimension q_dim <= num_col.
   * The diagonal of Q enters the primal step in closed form (proximal step), its off-diagonal part as an explicit
   * N x term (a third SpMV per trial; also sharded over several GPUs).  Entries above the diagonal, and a diagonal of the wrong sign
   * for the objective sense, are errors.  q_dim = 0 / NULL arrays = LP.  Through Highs::run() the QP case needs the
   * reference's QP gate lifted (integration/qp_gate_patch.py). */
  int32_t q_dim;
  int32_t reserved_q;
  const int32_t* q_start; /* [q_dim+1] */
  const int32_t* q_index; /* [q_start[q_dim]] row indices (>= column index: lower triangle) */
  const double* q_value;
} pdlp_problem_t;

/* Options, one field per entry that getUserParamsFromOptions
 * (CupdlpWrapper.cpp:642-717) forwards to cuPDLP-C. */
typedef struct pdlp_params {
  double primal_tol;      /* D_PRIMAL_TOL  <- primal_feasibility_tolerance | kkt_tolerance */
  double dual_tol;        /* D_DUAL_TOL    <- dual_feasibility_tolerance   | kkt_tolerance */
  double gap_tol;         /* D_GAP_TOL     <- pdlp_optimality_tolerance    | kkt_tolerance */
  double time_limit;      /* D_TIME_LIM    <- time_limit (seconds; +inf = none) */
  int32_t iter_limit;     /* N_ITER_LIM    <- pdlp_iteration_limit (clamped to int32) */
  int32_t features_off;   /* pdlp_features_off bitmask (scaling/restart/adaptive) */
  int32_t restart_method; /* pdlp_cupdlpc_restart_method; 0 disables restart */
  int32_t log_level;      /* 0 silent, 1 summary, 2 verbose (CupdlpWrapper.cpp:839-848) */
  /* --- MI355X-specific knobs (no reference counterpart) --- */
  int32_t device;         /* HIP device ordinal of this process (default 0) */
  int32_t check_interval; /* 0 = reference schedule (CUPDLP_RELEASE_INTERVAL 40) */
  int32_t reserved[2];    /* test-infrastructure switches (ignored by the product) */
  /* --- second reference path: solver="hipdlp" (HiPdlpWrapper.cpp, hipdlp/pdhg.cc:1783-1874) --- */
  int32_t algorithm;          /* 0 = cuPDLP-C path (solver="pdlp"), 1 = HiPDLP restarted Halpern PDHG */
  int32_t scaling_mode;       /* pdlp_scaling_mode bitmask: 1 Ruiz, 2 L2, 4 Pock-Chambolle (default 5) */
  int32_t ruiz_iterations;    /* pdlp_ruiz_iterations (default 10) */
  int32_t step_size_strategy; /* pdlp_step_size_strategy: 0 fixed; anything else = PID primal weight
                                 (HiGHS default 1 -> PID, pdhg.cc:1856-1864) */
  /* --- multi-GPU behind the one-call boundary (no reference counterpart: Ax_multi_gpu / ATy_multi_gpu
   *     are exit(1) stubs, cupdlp_linalg.c:420-423,453-456) --- */
  int32_t num_devices;        /* pdlp_mi355x_solve only: 0 = take PDLP_MI355X_DEVICES from the environment
                                 (default 1); G > 1 = the constraint matrix is row-block sharded over the
                                 devices device, device+1, ... device+G-1 of THIS process (one host thread
                                 per device, direct xGMI exchange through peer access) */
  int32_t updatable;          /* pdlp_mi355x_create: a bit mask of PDLP_UPDATABLE_*.  Non-zero = the solver takes
                                 pdlp_mi355x_update (it then keeps the scale factors of every scaling pass and the row kinds
                                 in HBM); with PDLP_UPDATABLE_MATRIX it also takes pdlp_mi355x_update_matrix (it then keeps
                                 the sparsity pattern in both orders, a source index per value slot of its layouts and the
                                 unscaled data as well: DESIGN.md section 2d has the bytes); with PDLP_UPDATABLE_HESSIAN it
                                 takes new Hessian values through pdlp_mi355x_update_values and keeps EVERY Hessian slot the
                                 caller passes; 0 = nothing is kept */
  /* --- log sink (HiGHS: highsLogUser).  NULL = stdout, as the reference's cuPDLP-C prints --- */
  void (*log_callback)(void* ctx, int level, const char* text); /* level 1 = summary, 2 = verbose */
  void* log_ctx;
} pdlp_params_t;

typedef struct pdlp_result {
  double* col_value; /* [num_col] caller-allocated, may be NULL */
  double* col_dual;  /* [num_col] */
  double* row_value; /* [num_row] */
  double* row_dual;  /* [num_row] */
  int32_t value_valid;
  int32_t dual_valid;
  int32_t term_code;   /* PDLP_TERM_* */
  int32_t term_iterate; /* 0 = last iterate, 1 = average iterate */
  int32_t num_iter;    /* outer PDHG iterations = highs_info.pdlp_iteration_count */
  int32_t num_trials;  /* trial steps incl. rejected ones (nStepSizeIter) */
  int32_t num_restarts;
  int32_t reserved_i;  /* HiPDLP path: 1 = stopped by the time limit (TerminationStatus::TIMEOUT) */
  /* cuPDLP's own view of the returned iterate (resobj, scaled-problem space
   * mapped back with row/col scale as in cupdlp_solver.c:12-204) */
  double primal_obj;
  double dual_obj;
  double primal_feas; /* ||r_p||_2 */
  double dual_feas;   /* ||r_d||_2 */
  double rel_gap;
  double norm_rhs;  /* ||b||_2 of the formulated, unscaled problem */
  double norm_cost; /* ||c||_2 */
  /* timings, seconds (steady clock; never time(NULL)) */
  double setup_seconds; /* formulate + scale + transpose + upload */
  double solve_seconds; /* PDHG loop */
  double reserved_d[4];
} pdlp_result_t;

typedef struct pdlp_mi355x_solver pdlp_mi355x_solver_t; /* opaque */

/* Fill *opt with the defaults HiGHS would pass for default options
 * (tolerances 1e-7, iteration limit INT32_MAX, time limit +inf, all features on). */
void pdlp_mi355x_default_params(pdlp_params_t* opt);

/* One-shot solve. Returns 0 on success (term_code says how it ended),
 * non-zero on failure (-> HighsStatus::kError / kSolveError). */
int pdlp_mi355x_solve(const pdlp_problem_t* P, const pdlp_params_t* opt,
                      pdlp_result_t* R);

/* Split form (what a long-lived Highs instance would hold). */
int pdlp_mi355x_create(const pdlp_problem_t* P, const pdlp_params_t* opt,
                       pdlp_mi355x_solver_t** out);
int pdlp_mi355x_run(pdlp_mi355x_solver_t* s, pdlp_result_t* R);
void pdlp_mi355x_destroy(pdlp_mi355x_solver_t* s);

/* Re-solve a held LP / QP after its costs, column bounds, row bounds or offset changed — the matrix, the Hessian (new
 * Hessian values go through pdlp_mi355x_update_values below), the sense, the sizes and the options stay.  Everything create() derives from the MATRIX (scale factors, row order,
 * slack columns, both orientations, slab layouts, tuning, the captured trial graph) is kept; the new data are brought
 * into the scaled standard form on the device by replaying the scale factors of every scaling pass in order, which
 * gives exactly the bits a fresh pdlp_mi355x_create on the modified problem has.
 *   * Only for solvers created with pdlp_params_t.updatable != 0, algorithm = 0, not sharded.
 *   * Values are taken as create takes them (|v| >= 1e20 is infinite; no check for NaN or crossed bounds).
 *   * Every row must keep its KIND (equality / >= / <= / ranged-or-free): the kind decides the row order, the slack
 *     columns and the sign of the row.  A change is refused; the message names the smallest such row and both kinds.
 *   * Everything is validated before anything is changed: after a non-zero return the solver is as it was.
 *   * Afterwards the solver is in the state of a fresh create on the modified problem; pdlp_mi355x_run may follow, and
 *     its pdlp_result_t.setup_seconds is the time the update took. */
typedef struct pdlp_update {
  const double* col_cost;   /* [num_col]  NULL = unchanged; original space, original sense */
  const double* col_lower;  /* [num_col]  NULL = unchanged */
  const double* col_upper;  /* [num_col]  NULL = unchanged */
  const double* row_lower;  /* [num_row]  NULL = unchanged; lower and upper are given together or not at all */
  const double* row_upper;
  double offset; int32_t has_offset; /* offset is taken only when has_offset != 0 */
  int32_t reserved;  /* pdlp_mi355x_batch_run: > 0 = this variant's iteration limit in place of opt->iter_limit; ignored elsewhere */
  /* start of the next run: all three NULL = cold start (as create without a hot start);
     all three given = hot start with the meaning of pdlp_problem_t.start_* when both valid flags are set */
  const double* start_col_value; const double* start_row_value; const double* start_row_dual;
} pdlp_update_t;
int pdlp_mi355x_update(pdlp_mi355x_solver_t* s, const pdlp_update_t* u);

/* pdlp_params_t.updatable: any non-zero value means PDLP_UPDATABLE_DATA */
enum {
  PDLP_UPDATABLE_DATA = 1,
  PDLP_UPDATABLE_MATRIX = 2, /* implies DATA */
  PDLP_UPDATABLE_HESSIAN = 4 /* implies DATA; independent of MATRIX */
};

/* Re-solve a held LP / diagonal-Hessian QP after the VALUES of its matrix changed, the sparsity pattern kept (through
 * HiGHS: Highs::changeCoeff on existing entries, then run()).  a_value[num_nz] in the caller's column-wise order, i.e.
 * the positions of pdlp_problem_t.a_value at create; an explicit 0.0 is a value like any other (create keeps them too).
 * u may be NULL or carry new costs / bounds / offset / start with the meaning and the checks of pdlp_mi355x_update; both
 * are applied as ONE change with one reset.  What create() derives from the PATTERN (row order, both orientations, slab
 * partitions and sorts, slab width, XCD map, pacing, task plans, the captured graph) is kept; what it derives from the
 * values (signs of <= rows, all scaling passes, the scaled data, max |a_ij|, the value arrays of the layouts) is redone
 * on the device by the set-up's own kernels.  Afterwards the solver is in the state of a fresh create on the problem
 * with these values and these data, bit for bit; pdlp_result_t.setup_seconds of the next run is the update's time.
 *   * Only for solvers created with PDLP_UPDATABLE_MATRIX in pdlp_params_t.updatable, algorithm = 0, not sharded, and
 *     no off-diagonal Hessian entries (their scaled copy follows the column factors) — unless the solver also has
 *     PDLP_UPDATABLE_HESSIAN, which keeps what rescales them: the call is then
 *     pdlp_mi355x_update_values(s, a_value, num_nz, NULL, 0, u).
 *   * num_nz must be the count at create, a_value non-NULL and not all zero (create refuses such a matrix).
 *   * Everything is validated before anything is changed: after a non-zero return the solver is as it was. */
int pdlp_mi355x_update_matrix(pdlp_mi355x_solver_t* s, const double* a_value, int64_t num_nz, const pdlp_update_t* u);

/* Re-solve a held QP after the VALUES of its Hessian changed, the sparsity pattern kept (through HiGHS: Highs::passHessian
 * on the same pattern, then run()) — a risk-aversion sweep, a re-estimated covariance, the Hessian of an SQP subproblem —
 * alone or together with new matrix values and new data, all applied as ONE change with one reset.
 *   * a_value == NULL (with num_nz == 0): the matrix is unchanged; else as pdlp_mi355x_update_matrix takes it (needs
 *     PDLP_UPDATABLE_MATRIX as well; a QP WITH off-diagonal Hessian entries is accepted here).
 *   * q_value == NULL (with num_q_nz == 0): the Hessian is unchanged; else q_value[num_q_nz] in the positions of
 *     pdlp_problem_t.q_value at create, num_q_nz == q_start[q_dim] at create.
 *   * u may be NULL, or carry data and a start with the meaning and the checks of pdlp_mi355x_update.
 * The scale factors come from the matrix alone, so with the matrix unchanged the new Hessian is brought into scaled form by
 * replaying the kept column factors of every pass: no scaling pass, no norm, no layout build, and the captured trial graph
 * stays.  With a_value the matrix update runs as above and the same replay, with the NEW factors, rescales the Hessian.
 * THE PATTERN CONTRACT.  A solver created with PDLP_UPDATABLE_HESSIAN keeps every Hessian slot the caller passes, explicit
 * zeros included (as a_value's are kept): its diagonal term exists iff the Hessian has any slot, its off-diagonal operand
 * iff the pattern has an off-diagonal slot; repeated (row, column) pairs are added left to right as always.  Without the
 * bit create drops zero values as before.  So a Hessian-updatable create differs from a plain one only where the caller
 * passes explicit zeros.
 *   * Only for solvers created with PDLP_UPDATABLE_HESSIAN, algorithm = 0, not sharded, and (for q_value) with a Hessian.
 *   * A diagonal that is negative after the objective sense is refused, with create's words and the smallest such column.
 *   * Everything is validated before anything is changed: after a non-zero return the solver is as it was.
 *   * Afterwards the solver is in the state of a fresh create on the modified problem with the same updatable bits, bit for
 *     bit; pdlp_result_t.setup_seconds of the next run is the update's time. */
int pdlp_mi355x_update_values(pdlp_mi355x_solver_t* s, const double* a_value, int64_t num_nz, const double* q_value,
                              int64_t num_q_nz, const pdlp_update_t* u);

/* ---- sessions: one resident solver reused across whole-problem solve calls ----------------------
 * A session takes a WHOLE problem on every call, as pdlp_mi355x_solve does, finds out on the device what differs from the
 * problem it holds and takes the cheapest path that gives the bits of a fresh solve: the caller neither tracks changes nor
 * chooses among pdlp_mi355x_update / _update_matrix / _update_values (through HiGHS: changeColCost / changeCoeff /
 * passHessian, then run() again).
 *
 * THE CONTRACT of pdlp_mi355x_session_solve(S, P, opt, R): *R is, bit for bit — every solution vector, every count, every
 * scalar except setup_seconds and solve_seconds — what
 *     pdlp_mi355x_create(P, opt') + pdlp_mi355x_run + pdlp_mi355x_destroy
 * gives, where opt' is opt with updatable |= PDLP_UPDATABLE_DATA | PDLP_UPDATABLE_MATRIX, and | PDLP_UPDATABLE_HESSIAN when P
 * has any Hessian slot (q_dim > 0 and q_start[q_dim] > 0).  That equals a plain pdlp_mi355x_solve(P, opt, R) except for a QP
 * whose caller passes explicit zeros in q_value: a Hessian-updatable create keeps every slot (THE PATTERN CONTRACT above),
 * a plain one drops zero values.  A hot start in P (both valid flags set) is honoured on every path.
 *
 * THE LADDER: on each call the first rule that applies decides pdlp_session_info_t.path.
 *   1. PDLP_SESSION_ONE_SHOT   opt->algorithm == 1, more than one device resolved (num_devices / PDLP_MI355X_DEVICES), or
 *                              sharding forced: those solvers refuse updates.  The call forwards to pdlp_mi355x_solve and the
 *                              session holds nothing afterwards.
 *   2. PDLP_SESSION_CREATE     nothing is held; a structural option differs (device, check_interval, features_off,
 *                              restart_method, algorithm, scaling_mode, ruiz_iterations, step_size_strategy, reserved[],
 *                              updatable); num_col, num_row, num_nz, sense, q_dim or the Hessian's slot count differ (so
 *                              also: a Hessian appears or disappears); a_start / a_index or q_start / q_index differ; some
 *                              row changes its kind (kind_row is the smallest such row; not an error).  What is held is
 *                              destroyed first.
 *   3. PDLP_SESSION_UPDATE_VALUES  q_value differs, with or without a_value and data.
 *   4. PDLP_SESSION_UPDATE_MATRIX  a_value differs, perhaps with data.
 *   5. PDLP_SESSION_UPDATE     only costs / bounds / offset differ, or nothing at all (then only the start and the reset).
 * Arrays are compared element by element on their 64-bit (32-bit) patterns: -0.0 differs from 0.0, NaNs compare as bits.  A
 * needless "changed" costs time only; a wrong "unchanged" cannot happen.  The run-time options primal_tol, dual_tol,
 * gap_tol, time_limit, iter_limit, log_level, log_callback, log_ctx are applied to the held solver on every path.  The
 * environment switches of a solver are read when it is created, as always.  If a reuse path fails
 * for any reason the held solver is destroyed and the create path is taken once; only a failure of that create is returned.
 * After a non-zero return the session holds nothing.  With log_level >= 1 one line names the path and the reason.
 *
 * What is kept in HBM besides the solver's own PDLP_UPDATABLE_* state: the caller's a_value, col_cost, col_lower, col_upper,
 * row_lower, row_upper and (QPs) q_start, q_index, q_value, plus staging of the same size (DESIGN.md section 2f has the
 * bytes; pdlp_session_info_t.held_bytes reports them).  The library keeps no host copy of the caller's problem.
 *
 * THREADING: a session is used by one thread at a time (different sessions may be used by different threads).
 * pdlp_mi355x_session_create makes no HIP call; create / release / destroy / info work on a machine without a GPU. */
enum {
  PDLP_SESSION_NONE = 0, /* nothing solved yet */
  PDLP_SESSION_CREATE = 1,
  PDLP_SESSION_UPDATE = 2,
  PDLP_SESSION_UPDATE_MATRIX = 3,
  PDLP_SESSION_UPDATE_VALUES = 4,
  PDLP_SESSION_ONE_SHOT = 5
};
/* pdlp_session_info_t.changed */
enum {
  PDLP_CHANGED_PATTERN = 1,          /* a_start / a_index */
  PDLP_CHANGED_MATRIX_VALUES = 2,    /* a_value */
  PDLP_CHANGED_HESSIAN_PATTERN = 4,  /* q_start / q_index */
  PDLP_CHANGED_HESSIAN_VALUES = 8,   /* q_value */
  PDLP_CHANGED_COST = 16,
  PDLP_CHANGED_COL_LOWER = 32,
  PDLP_CHANGED_COL_UPPER = 64,
  PDLP_CHANGED_ROW_BOUNDS = 128,     /* row_lower or row_upper */
  PDLP_CHANGED_OFFSET = 256,
  PDLP_CHANGED_RUNTIME_OPTIONS = 512,
  PDLP_CHANGED_STRUCTURAL_OPTIONS = 1024,
  PDLP_CHANGED_SHAPE = 2048          /* num_col, num_row, num_nz, sense, q_dim, Hessian slot count; arrays are then not compared */
};
typedef struct pdlp_session_info {
  int32_t path;     /* PDLP_SESSION_* of the last solve */
  int32_t changed;  /* PDLP_CHANGED_* against the held problem; 0 when nothing was held or the call was one-shot */
  int32_t kind_row; /* smallest row whose kind changes, or -1 */
  int32_t kind_was, kind_now; /* 0 equality, 1 <=, 2 >=, 3 ranged or free; -1 when kind_row is -1 */
  int32_t reserved;
  double diff_seconds;   /* uploads into staging + the comparison pass */
  double upload_seconds; /* of diff_seconds: the uploads alone (pageable host memory -> HBM) */
  double apply_seconds;  /* the chosen path's own work: the update from the staged arrays, or the create */
  double setup_seconds;  /* everything the call spent before the first iteration, the comparison included */
  int64_t held_bytes;   /* HBM the session keeps for reuse beyond a plain solver (0: nothing is held) */
  char reason[160];     /* NUL-terminated, e.g. "create: row 17 changes kind: equality -> <=" */
} pdlp_session_info_t;
typedef struct pdlp_mi355x_session pdlp_mi355x_session_t; /* opaque */
int pdlp_mi355x_session_create(pdlp_mi355x_session_t** out);
int pdlp_mi355x_session_solve(pdlp_mi355x_session_t* S, const pdlp_problem_t* P, const pdlp_params_t* opt, pdlp_result_t* R);
int pdlp_mi355x_session_info(const pdlp_mi355x_session_t* S, pdlp_session_info_t* out); /* about the last solve */
void pdlp_mi355x_session_release(pdlp_mi355x_session_t* S); /* drop the held solver, keep the session */
void pdlp_mi355x_session_destroy(pdlp_mi355x_session_t* S);
int64_t pdlp_mi355x_session_info_size(void); /* sizeof(pdlp_session_info_t); pdlp_mi355x_sizeof keeps its indices */

/* ---- batches: up to eight variants of one small LP solved at once, one per XCD ------------------
 * For callers with ONE matrix and MANY data sets (scenario sweeps, parametrics, the children of a branch-and-bound node).
 * A batch holds `lanes` (1..8) resident solvers of one problem P (algorithm 0, one device), each created as
 * pdlp_mi355x_create(P, opt') with opt' = opt | PDLP_UPDATABLE_DATA.  pdlp_mi355x_batch_run solves K >= 1 variants:
 * variant k is P with u[k] applied — meaning, checks and messages of pdlp_mi355x_update; u[k] may carry a start, and
 * u[k].reserved > 0 is an iteration limit of its own.  R[k] is caller-allocated as for pdlp_mi355x_run.
 *
 * THE CONTRACT: R[k] is, bit for bit — every solution vector, every count, every scalar except setup_seconds and
 * solve_seconds — what ONE held solver s, created with opt' on P (and with variant k's iteration limit), gives for
 * pdlp_mi355x_update(s, &u[k]) followed by pdlp_mi355x_run: by the update's own contract, a fresh create on the modified
 * problem.  For every K, every lane count and every order in which the variants happen to finish.
 *
 * Where the trial loop of P runs XCD-local (at most 32 work blocks: Netlib-class LPs) the lanes' loops and checks share
 * launches, lane L on XCD L, and a lane whose variant has ended takes the next one while the others carry on.  Nothing is
 * synchronised between variants; time and iteration limits count per variant, from its own start.  Everywhere else
 * batch_run is a loop of update + run on one lane; pdlp_batch_info_t.reason says which, and why.
 *   * All u[k] are validated before anything is changed; a refusal names the variant ("variant 3: ...", then update's
 *     words) and leaves the batch as it was.
 *   * HiPDLP, more than one device, forced sharding and lanes outside 1..8 are refused at create, before any device call.
 *   * A lane whose workgroups of a shared launch were not placed on one XCD, not resident together or did not meet at a
 *     barrier leaves the shared launches for good; its variant is re-solved alone through the ordinary run
 *     (fallback_variants counts them).
 *   * With log_level >= 1 every log line carries a "[variant k] " prefix.
 *
 * VALUE VARIANTS (pdlp_mi355x_batch_run_values): a variant may also carry new MATRIX values and new HESSIAN values on P's
 * patterns — a risk-aversion sweep or re-estimated covariances on one portfolio model, scenario LPs whose coefficients
 * differ on one pattern, SQP subproblems.  The lanes' updatable bits are the caller's: the batch adds none besides DATA,
 * so a_value needs PDLP_UPDATABLE_MATRIX in opt and q_value needs PDLP_UPDATABLE_HESSIAN — and lanes created with
 * PDLP_UPDATABLE_HESSIAN follow THE PATTERN CONTRACT above (every slot the caller passes is kept, explicit zeros included).
 * It is batch_run's contract with one change: R[k] is, bit for bit, what the ONE held solver s gives for the update below
 * followed by pdlp_mi355x_run, where A_k is v[k].a_value where given and P's a_value otherwise, Q_k likewise:
 *     neither array ....................................... pdlp_mi355x_update(s, &v[k].u)
 *     a_value only, opt without PDLP_UPDATABLE_HESSIAN ..... pdlp_mi355x_update_matrix(s, A_k, num_nz, &v[k].u)
 *     otherwise ........................................... pdlp_mi355x_update_values(s, A_k, nnz, Q_k, qnz, &v[k].u)
 * "Unchanged" in a batch always means P's values, whatever variant the lane solved before: an array that a lane's earlier
 * variant changed and this one leaves alone goes back to P's in the same update.  (A count given with a NULL array sends
 * the variant to update_values, which refuses it.)  All v[k] are validated before anything is changed — the all-zero
 * matrix and the negative diagonal included —; a refusal reads "variant k: " + the words of the entry the variant maps to
 * and leaves the batch as it was.  pdlp_batch_info_t describes a batch_run_values as it does a batch_run; value updates
 * change no pattern, so whether the lanes share launches is the same for both entries.
 * THREADING: one thread uses a batch at a time. */
typedef struct pdlp_batch_info { /* about the last pdlp_mi355x_batch_run */
  int32_t lanes;             /* solvers held */
  int32_t lanes_concurrent;  /* how many ran inside shared launches at once; 1 = one after the other */
  int32_t variants;
  int32_t trial_launches;    /* shared launches issued: trial loops, */
  int32_t check_launches;    /* checks */
  int32_t fallback_variants; /* variants re-solved alone after their lane left the shared launches */
  int32_t xcc_of_lane[8];    /* the XCC id each lane's workers published, or -1 */
  int32_t reserved[2];
  double wall_seconds;
  char reason[160];          /* NUL-terminated, e.g. "concurrent: 8 lanes, 21 workgroups each" or
                                "sequential: 48 work blocks need more than one XCD" */
} pdlp_batch_info_t;
typedef struct pdlp_mi355x_batch pdlp_mi355x_batch_t; /* opaque */
int pdlp_mi355x_batch_create(const pdlp_problem_t* P, const pdlp_params_t* opt, int32_t lanes, pdlp_mi355x_batch_t** out);
int pdlp_mi355x_batch_run(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_update_t* u, pdlp_result_t* R);
typedef struct pdlp_variant {
  const double* a_value; int64_t num_nz;    /* NULL / 0: the matrix values of the batch's problem P */
  const double* q_value; int64_t num_q_nz;  /* NULL / 0: P's Hessian values */
  pdlp_update_t u;                          /* data, start, u.reserved = iteration limit; all zero: P's data, cold start */
} pdlp_variant_t;
int pdlp_mi355x_batch_run_values(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_variant_t* v, pdlp_result_t* R);
int64_t pdlp_mi355x_variant_size(void);     /* sizeof(pdlp_variant_t); pdlp_mi355x_sizeof keeps its indices */
int pdlp_mi355x_batch_info(const pdlp_mi355x_batch_t* B, pdlp_batch_info_t* out);
void pdlp_mi355x_batch_destroy(pdlp_mi355x_batch_t* B);
int64_t pdlp_mi355x_batch_info_size(void); /* sizeof(pdlp_batch_info_t); pdlp_mi355x_sizeof keeps its indices */

/* ---- pools: up to eight DIFFERENT small LPs solved at once, one per XCD ----------------------------
 * For callers with MANY small problems (a Netlib sweep, decomposition subproblems, per-scenario models whose coefficients
 * differ, a queue of user models).  One call, no handle, nothing held afterwards: P[0..K) are solved with the options opt
 * (algorithm 0, one device) on `lanes` (1..8) lanes; R[k] is caller-allocated as for the one-call solve.
 *
 * THE CONTRACT: R[k] is, bit for bit — every solution vector, every count, every scalar except setup_seconds and
 * solve_seconds — what a solver created for P[k] with opt gives for one run: create, run, destroy.  For every K, every lane
 * count, every order of the problems and every order in which they happen to finish.  A hot start in P[k] is honoured;
 * P[i] == P[j] is allowed.
 *
 * Problems are taken in the caller's order: a free lane creates the next problem's solver (at most lanes + 1 solvers
 * exist at a time; a finished one is destroyed before its lane refills).  Where that solver's trial loop runs XCD-local (at
 * most 32 work blocks: Netlib-class LPs) it joins the shared launches of the batches, lane L on XCD L, with a grid and a
 * number of barriers per trial of its own (PDLP_POOL_SHARED).  A solver that does not qualify — a larger LP — is run right
 * there in the ordinary way (PDLP_POOL_ALONE; pdlp_pool_info_t.reason holds the reason of the first one) while the lanes
 * wait.  lanes == 1 or K == 1 is a loop of ordinary solves.
 *   * Refused before any device call, R and path untouched: null arguments, K < 1, lanes outside 1..8, HiPDLP, more than
 *     one device, forced sharding, and any P[k] that the one-call solve refuses as malformed or that has more than
 *     INT32_MAX nonzeros ("problem 3: ...", then the existing words).
 *   * If a create or a solve fails, the call ends there: every solver is destroyed, the return value is non-zero and the
 *     message names the problem ("problem k: ...").  R[j] of the problems finished by then stay valid: path[j] != 0.
 *   * opt->time_limit counts per problem from the start of ITS solve (behind its create), and includes the time its lane
 *     waited while another problem was created or run alone.  A solve that ends by its time limit is outside the contract,
 *     as everywhere.
 *   * A lane whose workgroups of a shared launch were not placed on one XCD, not resident together or did not meet at a
 *     barrier leaves the shared launches for good; its problem is re-solved alone once the others have finished
 *     (PDLP_POOL_FALLBACK).
 *   * With log_level >= 1 every log line carries a "[problem k] " prefix.
 * THREADING: as the one-call solve. */
enum { PDLP_POOL_NOT_RUN = 0, PDLP_POOL_SHARED = 1, PDLP_POOL_ALONE = 2, PDLP_POOL_FALLBACK = 3 };
typedef struct pdlp_pool_info {
  int32_t problems, lanes;
  int32_t lanes_concurrent;   /* most problems inside shared launches at once; 1 = one after the other */
  int32_t shared_problems;    /* solved inside shared launches */
  int32_t alone_problems;     /* did not qualify (reason of the first one in `reason`): ordinary run */
  int32_t fallback_problems;  /* left the shared launches by the failure rule, re-solved alone */
  int32_t trial_launches, check_launches;
  int32_t mixed_launches;     /* trial launches that carried 2-barrier and 3-barrier lanes together */
  int32_t xcc_of_lane[8];     /* the XCC id the last problem finished on each lane published, or -1 */
  int32_t reserved[3];
  double wall_seconds, create_seconds; /* create_seconds: sum over the problems' creates */
  char reason[160];           /* NUL-terminated: "concurrent: 8 lanes", "sequential: one lane", or why the first problem
                                 that ran alone did, e.g. "42 work blocks need more than one XCD" */
} pdlp_pool_info_t;
int pdlp_mi355x_solve_many(int32_t K, const pdlp_problem_t* const* P, const pdlp_params_t* opt, int32_t lanes,
                           pdlp_result_t* R, int32_t* path /* [K] PDLP_POOL_*, may be NULL */,
                           pdlp_pool_info_t* info /* may be NULL */);
int64_t pdlp_mi355x_pool_info_size(void); /* sizeof(pdlp_pool_info_t); pdlp_mi355x_sizeof keeps its indices */

/* ---- device-resident entries: problems, updates and solutions as arrays already in HBM -------------
 * For callers that produce the next problem's data on the GPU and read the solution there (successive linear programming,
 * SQP, MPC, scenario sweeps, a training loop around an LP / QP layer): nothing bounces through host memory.  The structs
 * above are reused; in these entries EVERY ARRAY POINTER inside them is a pointer into HBM ON THE SOLVER'S DEVICE
 * (pdlp_params_t.device), scalars and the struct itself stay in host memory.
 *
 * stream: the hipStream_t (as void*) on which the caller produced the arrays; the library orders its own stream behind an
 * event recorded there and never synchronises the caller's stream.  NULL: the arrays are complete, or were produced on the
 * default stream (the event is then recorded there).  The caller's arrays are read-only, and may be reused or freed as soon
 * as the call returns; results are complete when the call returns.
 *
 * THE POINTER CHECK: before its first launch or copy each entry asks the runtime about every non-NULL array pointer it was
 * given (hipPointerGetAttributes).  Host memory — pageable, pinned or registered —, managed memory and another device's
 * memory are refused: non-zero return, pdlp_mi355x_last_error names the field ("pdlp_mi355x_update_device: col_cost is not
 * device memory on device 0"), the solver stays as it was.
 *
 * pdlp_mi355x_create_device: the solver is, bit for bit, the one pdlp_mi355x_create gives for the same problem in host arrays
 * with the same opt.  Algorithm 0 on one device: HiPDLP, num_devices > 1 and forced sharding are refused before any device
 * call.  Always the device-side set-up; the library downloads a_start, col_cost, row_lower, row_upper, q_start and a hot
 * start (O(num_col + num_row): the monotone checks and the left-to-right norms are the host's), never a_index, a_value,
 * q_index or q_value — a row index out of range, an entry above the diagonal, an all-zero matrix are found by kernels and
 * refused in pdlp_mi355x_create's words.  A Hessian whose q_start does not run from 0 without decreasing is refused.
 *
 * pdlp_mi355x_update_device: ONE entry for the three updates, routed as pdlp_mi355x_batch_run_values routes a variant —
 *     neither array ................................................ pdlp_mi355x_update(s, u)
 *     a_value only, a solver without PDLP_UPDATABLE_HESSIAN ......... pdlp_mi355x_update_matrix(s, a_value, num_nz, u)
 *     otherwise .................................................... pdlp_mi355x_update_values(s, a_value, num_nz, q_value, num_q_nz, u)
 * with that entry's checks, order, words (behind "pdlp_mi355x_update_device: ") and all-or-nothing rule; afterwards the
 * solver has the bits that entry gives for the same arrays in host memory.  The staging copy is device to device; costs,
 * row bounds and a start are also downloaded (the ordered norms, the kind-change message, the start's formulation).
 *
 * pdlp_mi355x_run_device: pdlp_mi355x_run with the four vectors of R in HBM: the loop is the same, the post-solve runs as
 * kernels and gives the bits of the host's.  A NULL vector is skipped; value_valid, dual_valid, every count and scalar are
 * written to the host struct as always.  Sharded solvers are refused.  The entry takes no stream: whatever the caller has
 * queued that still READS the vectors of R (the previous solution, where a loop reuses its buffers) must have completed
 * before the call — the post-solve overwrites them on the library's own stream.
 *
 * SIZES are the caller's contract, as in every other entry: the pointer check establishes where an array lives, not how
 * long it is; each array must hold the count its field's comment gives.
 *
 * The solver does not remember where its problem came from: host and device entries mix freely on one solver. */
int pdlp_mi355x_create_device(const pdlp_problem_t* P_dev, const pdlp_params_t* opt, void* stream, pdlp_mi355x_solver_t** out);
int pdlp_mi355x_update_device(pdlp_mi355x_solver_t* s, const double* a_value_dev, int64_t num_nz, const double* q_value_dev,
                              int64_t num_q_nz, const pdlp_update_t* u_dev, void* stream);
int pdlp_mi355x_run_device(pdlp_mi355x_solver_t* s, pdlp_result_t* R_dev);
/* pdlp_mi355x_batch_run_device: pdlp_mi355x_batch_run_values with the variants' arrays and the solutions' vectors in HBM on
 * the batch's device — for callers that hold K cost vectors or K sets of matrix / Hessian values as a [K, n] tensor and want
 * [K, n] solutions back on the device.  v_dev[k] and R_dev[k] are host structs; every array pointer
 * inside them follows the rule above.  `stream` has update_device's meaning: every lane's stream is ordered behind ONE event
 * recorded there, and it is never synchronised; NULL is the default stream.  R_dev follows run_device's rule: a NULL vector
 * is skipped, whatever the caller has queued that still READS the vectors of R_dev must have completed before the call,
 * counts and scalars go to the host structs.  A hot start inside a variant is taken as update_device takes it (downloaded).
 *
 * THE CONTRACT: R_dev[k] holds, bit for bit — every solution vector, every count, every scalar except setup_seconds and
 * solve_seconds — what pdlp_mi355x_batch_run_values gives for the same arrays in host memory on the same batch; for every
 * K, every lane count, every finishing order, where the lanes share launches and where they do not.  pdlp_batch_info_t
 * describes the call as it does a batch_run_values.  "Unchanged" means P's values here too: the batch uploads a copy of
 * P's data at its first device run and restores from there.  Host and device runs mix freely on one batch.
 *
 * REFUSALS are all-or-nothing (the batch stays as it was) and come in a fixed order:
 *   1. without any device call: null arguments and K < 1; then, for k = 0..K-1, what the entry variant k maps to refuses
 *      without looking at a value (shape, counts, updatable bits, partial start): "variant k: " + that entry's words;
 *   2. THE POINTER CHECK on every array of every variant, then on every vector of every result, before any launch or copy
 *      touches a caller's array: "variant 5: col_cost is not device memory on device 0", "result 2: row_dual is not ...";
 *   3. the value checks, on the device, for all K variants in ONE launch: the lowest k with a finding is refused; within
 *      it the order is row-kind change, all-zero matrix, negative diagonal: "variant k: " + the words the update entries
 *      use (for the kind-change message that one row's two bounds are downloaded). */
int pdlp_mi355x_batch_run_device(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_variant_t* v_dev, pdlp_result_t* R_dev,
                                 void* stream);
/* ONE HIP RUNTIME PER PROCESS: the caller's arrays and this library must live in the same copy of the HIP runtime.  A
 * process that holds two — a PyTorch wheel bundles its own libamdhip64 — has the GPU in whichever started first; the other
 * finds no device ("no HIP device available").  highs_amd.solver.lib() registers the system's copy under the name a later
 * `import torch` asks for, so both share it. */

/* Host-only restatement of the session's decision for the CPU tests: `held` / held_opt are the problem and options of the
 * previous call (held == NULL: nothing is held), P / opt those of this one.  Same ladder (one function shared with the
 * session), same changed mask, same reason words; the four timings and held_bytes are 0. */
int pdlp_mi355x_host_classify(const pdlp_problem_t* held, const pdlp_params_t* held_opt, const pdlp_problem_t* P,
                              const pdlp_params_t* opt, pdlp_session_info_t* out);

/* The same two entries with 64-bit column starts (HighsInt = int64_t builds, or any caller whose matrix
 * starts are 64-bit): a_start64[num_col+1] replaces P->a_start, which is ignored and may be NULL; every
 * other field keeps its meaning.  a_start64 is checked on the host before any HIP call: a_start64[0] == 0,
 * never decreasing, a_start64[num_col] == num_nz, and every row index in range.  A problem that passes
 * behaves exactly as through pdlp_mi355x_create / pdlp_mi355x_solve.  The device path indexes the
 * formulated matrix with 32-bit offsets, so a problem with more than INT32_MAX nonzeros is refused with
 * a message that names the count, the limit and the path (algorithm, num_devices) that refused it. */
int pdlp_mi355x_create_wide(const pdlp_problem_t* P, const int64_t* a_start64,
                            const pdlp_params_t* opt, pdlp_mi355x_solver_t** out);
int pdlp_mi355x_solve_wide(const pdlp_problem_t* P, const int64_t* a_start64,
                           const pdlp_params_t* opt, pdlp_result_t* R);

/* ---- measurement / parity hooks (device-resident state) ----------------
 * These exist so that tests and bench.py can drive and observe the hot loop
 * with all inputs already resident in HBM. They are not needed by HiGHS. */

/* Formulated sizes: n = nCols (incl. slack columns), m = nRows, nnz, nEqs. */
int pdlp_mi355x_dims(const pdlp_mi355x_solver_t* s, int32_t* n_cols,
                     int32_t* n_rows, int64_t* nnz, int32_t* n_eqs);

/* (Re)initialise step sizes and iterates: PDHG_Init_Step_Sizes + PDHG_Init_Variables. */
int pdlp_mi355x_reset(pdlp_mi355x_solver_t* s);

/* Run exactly n_iters accepted PDHG iterations starting from the current
 * state, following the reference's check/restart schedule but never
 * terminating on optimality (fixed work for timing). Reports the number of
 * trial steps taken and the GPU time of the loop measured with HIP events on
 * the solver's stream. */
typedef struct pdlp_iter_stats {
  int32_t iters;
  int32_t trials;
  int32_t checks;
  int32_t restarts;
  double gpu_ms;      /* hipEvent elapsed over the whole loop on the solver stream */
  double wall_ms;     /* host steady clock over the same region */
  double spmv_ax_ms;  /* filled only when profiling is enabled, else 0 */
  double spmv_aty_ms;
  double reserved[4];
} pdlp_iter_stats_t;
int pdlp_mi355x_iterate(pdlp_mi355x_solver_t* s, int32_t n_iters,
                        pdlp_iter_stats_t* st);

/* Device vector access by name for kernel-level parity tests. Names:
 * "x","y","ax","aty" (current iterate), "x_next","y_next","ax_next","aty_next",
 * "x_avg","y_avg","ax_avg","aty_avg","x_sum","y_sum","cost","rhs","lower",
 * "upper","col_scale","row_scale","slack_pos","slack_neg"; QP solvers also "qdiag" (the scaled diagonal of Q, length n).
 * len must equal the vector's length (n or m).  Setting "lower" or "upper" also refreshes the per-block bound
 * scalars of the fused trial (and captures its graph again where the one-lower-bound instantiation changes). */
int pdlp_mi355x_get_vector(pdlp_mi355x_solver_t* s, const char* name,
                           double* host, int64_t len);
int pdlp_mi355x_set_vector(pdlp_mi355x_solver_t* s, const char* name,
                           const double* host, int64_t len);

/* Run one named kernel stage on the current device state. Stages:
 *  "ax"        ax      = A x            (CSR SpMV,  cupdlp_linalg.c:460 Ax)
 *  "aty"       aty     = A' y           (CSC SpMV,  cupdlp_linalg.c:496 ATy)
 *  "trial"     one trial step with the current step sizes (cupdlp_step.c:241-257)
 *  "residuals" PDHG_Compute_Residuals on current+average (cupdlp_solver.c:473)
 *  "profile_on" / "profile_off"  bracket the two SpMV launches of every trial with HIP events
 *              (eager launches, no hipGraph): the next pdlp_mi355x_iterate then reports the
 *              IN-LOOP average launch durations in spmv_ax_ms / spmv_aty_ms (reserved[0] = launches)
 *  "exchange"  scalars_out[0] = 0 not sharded, 1 RCCL all-reduce, 2 direct xGMI mesh
 *  "fused_form" launches nothing: the instantiation of the fused A'y+ launch this solver runs —
 *              [0] 1 = the 2-launch (fused) trial, [1] 1 = its 64-register variant with co-resident task
 *              workgroups (TWO), [2] CC, [3] ULO (one lower bound for all columns), [4] task workgroups,
 *              [5] 1 = the streaming blocks run the long columns' tasks themselves, [6] 1 = the tail columns
 *              are touched before the barrier, [7] accumulator rows per block of A' in the slab layout,
 *              [8] bytes of the state record in the launch's LDS request
 * HiPDLP solvers (algorithm = 1) instead know:
 *  "steps"     scalars_out[0] holds k on entry (1..40): run Halpern steps 1..k of a block, first and
 *              last one "major" (pdhg.cc:961-1018), from the current state and step sizes
 *  "block"     one whole block of 40 steps, then scalars_out[0] = fixed-point error (pdhg.cc:709-739)
 * scalars_out receives stage-specific scalars, n_scalars its capacity. */
int pdlp_mi355x_stage(pdlp_mi355x_solver_t* s, const char* stage,
                      double* scalars_out, int32_t n_scalars);

/* Time `reps` launches of one kernel with HIP events on the solver stream;
 * returns average milliseconds per launch in *avg_ms. Kernels: "spmv_ax",
 * "spmv_aty", "primal_step", "trial" (whole trial sequence), "copy" (n+m doubles
 * device copy, the measured HBM ceiling). */
int pdlp_mi355x_time_kernel(pdlp_mi355x_solver_t* s, const char* kernel,
                            int32_t reps, double* avg_ms);

/* Multi-GPU (row-block sharding): the process owning rank r of
 * world w passes the FULL problem; create() keeps only its row block.
 * id is the 128-byte communicator id obtained on rank 0 with
 * pdlp_mi355x_comm_unique_id and broadcast by the caller (torch.distributed /
 * MPI / anything).  All ranks must be processes of ONE node: the n-vector
 * exchange writes directly into the peers' HIP-IPC-mapped device memory over
 * xGMI; the id names their rendezvous and is also a valid
 * ncclUniqueId for the RCCL all-reduce fallback.  run/iterate/stage("residuals")
 * are collective afterwards.  Both algorithms shard (algorithm = 1 over the direct
 * exchange only). */
int pdlp_mi355x_comm_unique_id(void* id128);
int pdlp_mi355x_create_sharded(const pdlp_problem_t* P, const pdlp_params_t* opt,
                               int32_t rank, int32_t world, const void* id128,
                               pdlp_mi355x_solver_t** out);

/* Synthetic LP generator of SURVEY §8d / BASELINE.md §3 (std::mt19937_64(seed),
 * box 0<=x<=1, k = nnz/m draws per row, even rows equalities, odd rows <=).
 * One call: *P_out is filled with arrays malloc'ed by the library (release them with
 * pdlp_mi355x_free_problem).  Returns 1 on bad arguments (P_out == NULL, m or n <= 0, nnz_target < m) or
 * when memory runs out; never throws. */
int pdlp_mi355x_gen_synthetic(int32_t m, int32_t n, int64_t nnz_target,
                              uint64_t seed, pdlp_problem_t* P_out);
void pdlp_mi355x_free_problem(pdlp_problem_t* P);

/* ---- host-only introspection (no GPU needed) ---------------------------
 * The standard form the device iterates on: formulate (CupdlpWrapper.cpp:280-448)
 * + scaling (cupdlp_scaling.c) + both matrix orientations (cupdlp_utils.c:1222).
 * Used by the CPU test-suite to check the host logic against the oracle and
 * by the multi-GPU tests to check the row-block partition.  Arrays are
 * malloc'ed by the library; release with pdlp_mi355x_free_prepared. */
typedef struct pdlp_prepared {
  int32_t n, m, n_eqs, n_orig;
  int64_t nnz;
  int32_t *csr_beg, *csr_idx; /* rows, ascending column */
  double* csr_val;
  int32_t *csc_beg, *csc_idx; /* columns, ascending row */
  double* csc_val;
  double *cost, *rhs, *lower, *upper, *col_scale, *row_scale;
  int32_t *row_kind, *row_new_idx; /* per original row */
  double norm_cost, norm_rhs, mat_norm_inf;
  int32_t spmv_blocks_ax, spmv_blocks_aty; /* CSR-adaptive work blocks */
} pdlp_prepared_t;
int pdlp_mi355x_host_prepare(const pdlp_problem_t* P, const pdlp_params_t* opt,
                             pdlp_prepared_t* out);
/* Host restatement of pdlp_mi355x_update for the CPU tests: prepares P as host_prepare does, keeping the scale factors of
 * every pass, applies u by the same replay (same validation, same messages: opt->updatable = 0 and algorithm = 1 are
 * refused here too) and returns the standard form — which must equal host_prepare of the modified problem bit for bit. */
int pdlp_mi355x_host_prepare_updated(const pdlp_problem_t* P, const pdlp_params_t* opt, const pdlp_update_t* u,
                                     pdlp_prepared_t* out);
/* Host restatement of pdlp_mi355x_update_matrix for the CPU tests, as the entry above is for update: prepares P, keeping
 * the pattern, the passes and the unscaled data, then applies a_value (positions of P->a_value) and u (may be NULL) as the
 * device does — same validation, same messages. */
int pdlp_mi355x_host_prepare_updated_matrix(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value,
                                            const pdlp_update_t* u, pdlp_prepared_t* out);
void pdlp_mi355x_free_prepared(pdlp_prepared_t* out);
/* Host twin of a Hessian-updatable create and of pdlp_mi355x_update_values, for the CPU tests.  a_value, q_value and u all
 * NULL: a plain prepare of P (with the pattern contract iff opt->updatable has PDLP_UPDATABLE_HESSIAN).  Otherwise P is
 * prepared keeping what the device keeps and the change is applied as the device applies it — same validation, same
 * messages.  *qout receives the scaled Hessian of the form: its diagonal (has_diag = 0: none) and its off-diagonal part
 * with both triangles, by rows with ascending column.  Arrays are malloc'ed by the library; release with
 * pdlp_mi355x_free_prepared / pdlp_mi355x_free_prepared_hessian. */
typedef struct pdlp_prepared_hessian {
  int32_t n, has_diag;
  int64_t nnz_off;
  double* qdiag;           /* [n] or NULL */
  int32_t *q_beg, *q_idx;  /* [n+1], [nnz_off] or NULL */
  double* q_val;
} pdlp_prepared_hessian_t;
int pdlp_mi355x_host_prepare_qp(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value, const double* q_value,
                                const pdlp_update_t* u, pdlp_prepared_t* out, pdlp_prepared_hessian_t* qout);
void pdlp_mi355x_free_prepared_hessian(pdlp_prepared_hessian_t* out);
/* Row-block partition used by create_sharded: offsets[world+1]. */
int pdlp_mi355x_row_partition(const pdlp_prepared_t* prep, int32_t world,
                              int32_t* offsets);
/* The slab layout the GPU SpMV uses for large operands (see DESIGN.md "slab SpMV"), built on the
 * host for inspection by the CPU tests: which = 0 for A (rows), 1 for A' (columns).  Free with
 * pdlp_mi355x_free_slab_layout. */
typedef struct pdlp_slab_layout {
  int32_t rows_per_block; /* the most majors any block owns (size of the LDS accumulators) */
  int32_t rows_per_wave;  /* reserved (0): waves own variable runs of majors, see wave_beg */
  int32_t n_blocks, minor_bits, slab_width_log2, n_long;
  int64_t nnz_short;
  int32_t* wave_ptr;  /* [16*n_blocks+1] entry offsets */
  uint32_t* ent;      /* [nnz_short] (local_major << minor_bits | minor), local = major - first major of the owning wave */
  double* val;        /* [nnz_short] */
  uint32_t* long_mask;/* [n_major/32 + 1] bit r: major r is a long one */
  int32_t* long_map;  /* [n_long] */
  int32_t* wave_beg;  /* [16*n_blocks+1] first major of every wave: blocks and waves are cut by work, not by major
                         count (csrc/pdlp_host.hpp slabPartition holds the rule) */
} pdlp_slab_layout_t;
int pdlp_mi355x_host_slab_layout(const pdlp_prepared_t* prep, int32_t which,
                                 int32_t long_limit, pdlp_slab_layout_t* out);
void pdlp_mi355x_free_slab_layout(pdlp_slab_layout_t* out);
/* The segment tasks of that operand's long majors (more than long_limit entries) as the slab SpMV launches run them
 * (csrc/pdlp_host.hpp planSlabTasks): task t belongs to task workgroup t / task_group, which is workgroup
 * n_blocks + t / task_group of its launch and runs on XCD (n_blocks + t / task_group) % 8; a task is dealt to a workgroup
 * of the XCD whose streaming blocks gather from the stretch of the vector its entries lie in (tile_owner).  For the CPU
 * tests; balance = 1: at least one task workgroup per CU.  Free with pdlp_mi355x_free_task_plan. */
typedef struct pdlp_task_plan {
  int32_t n_tasks, task_group, n_seg_slots, n_long, n_blocks, tile_log2, n_tiles, reserved;
  int32_t* tasks;     /* [8*n_tasks] entry range [p_beg, p_end) in long_idx, long-major index c (-1: idle), first
                         segment-sum slot of the major, its segment count, its index in the result vector, contained,
                         segment number */
  int8_t* tile_owner; /* [n_tiles] XCD (contiguous block -> XCD map) that gathers most from minors [t << tile_log2, ...) */
  int32_t* long_beg;  /* [n_long+1] compact CSR of the long majors */
  int32_t* long_idx;  /* [long_beg[n_long]] */
} pdlp_task_plan_t;
int pdlp_mi355x_host_task_plan(const pdlp_prepared_t* prep, int32_t which, int32_t long_limit, int32_t balance,
                               pdlp_task_plan_t* out);
void pdlp_mi355x_free_task_plan(pdlp_task_plan_t* out);
/* exp(x[i]) and log(x[i]) as the solver computes them in the restart's primal-weight update (plain IEEE arithmetic,
 * csrc/pdlp_detmath.h: the same bits on host and device) — for the CPU tests, which compare them with long-double libm
 * and with the oracle's separately written restatement.  Reference arithmetic: cupdlp_step.c:165-170 (libm). */
void pdlp_mi355x_det_exp_log(int32_t n, const double* x, double* exp_out, double* log_out);
/* ---- MPS ingest (host-only, no GPU needed) --------------------------------------
 * Multi-threaded reader of free-format MPS files (fixed-format files without spaces in names are free
 * format too).  Replaces, for such files, the reference's single-threaded parser
 *   io/FilereaderMps.cpp:24-58 -> free_format_parser::HMpsFF::loadProblem (io/HMpsFF.cpp:21-133)
 * and builds the same model: first N row = objective (other N rows dropped), duplicate row / column names
 * are distinct rows / columns and only the first occurrence can be addressed, undefined rows and repeated
 * (column, row) pairs are ignored with a warning, zero coefficients dropped, entries of a column in file
 * order, RHS of the cost row = -offset, RANGES by sign, integer columns of a MARKER block are [0,1] until
 * a bound says otherwise, BOUNDS may introduce columns, QUADOBJ / QMATRIX -> Hessian, OBJSENSE either style.
 * integration/FilereaderMpsMi355x.cpp shows the binding inside Highs::readModel.
 * Return: 0 ok (out filled; release with pdlp_mi355x_free_mps_model), 1 malformed file / unsupported
 * section (pdlp_mi355x_last_error), 2 file cannot be opened, 3 names contain spaces: a fixed-COLUMN reader
 * is needed (FreeFormatParserReturnCode::kFixedFormat — the reference then falls back to io/HMPSIO.cpp),
 * 4 the file is a gzip stream and libz could not be loaded (gzip files are inflated by the reader itself otherwise,
 * as the reference does through zstr when built with zlib, HMpsFF.cpp:253-261). */
typedef struct pdlp_mps_model {
  pdlp_problem_t lp;           /* HighsLp fields; lp.q_* = LOWER TRIANGLE of the Hessian (what this library's
                                  QP path and HighsHessian::kTriangular expect), NULL / 0 for an LP */
  int32_t cost_row_location;   /* lp.cost_row_location_ (HMpsFF.cpp:639) */
  int32_t num_integrality;     /* 0: every column continuous (lp.integrality_ stays empty), else num_col */
  const uint8_t* integrality;  /* HighsVarType per column: 0 continuous, 1 integer, 2 semi-continuous, 3 semi-integer */
  const char* model_name;      /* NAME line */
  const char* objective_name;  /* name of the cost row ("Objective" if none) */
  /* names: one pool of NUL-terminated strings + [num+1] start offsets; NULL when the file repeats a name
   * (the reference clears its name arrays then, HMpsFF.cpp:63-80) */
  const char* col_name_pool;
  const int64_t* col_name_start;
  const char* row_name_pool;
  const int64_t* row_name_start;
  /* the Hessian exactly as the parser leaves it (square, column-wise, file order: fillHessian, HMpsFF.cpp:177-216) */
  int32_t hessian_dim;
  int32_t warning_issued;      /* HMpsFF::warning_issued_ at the end of the read: FilereaderRetcode::kWarning if set.
                                  (The reference ASSIGNS the flag at the end of COLUMNS / RHS / BOUNDS / RANGES, so
                                  earlier warnings may be forgotten; num_warnings below counts every class met.) */
  const int32_t* hessian_start;
  const int32_t* hessian_index;
  const double* hessian_value;
  int32_t num_warnings;        /* warning classes met */
  int32_t threads;             /* host threads used */
  const char* warnings;        /* one line per warning class */
  int64_t file_bytes;
  double seconds;              /* wall time of the call */
} pdlp_mps_model_t;
/* num_threads <= 0: one per hardware thread (at least 1 MB of file each, at most 64); > 0: exactly that many. */
int pdlp_mi355x_read_mps(const char* path, int32_t num_threads, pdlp_mps_model_t* out);
/* The same with HMpsFF::time_limit_ (io/FilereaderMps.cpp:30-31, io/HMpsFF.cpp:218-220): seconds from the start of
   the call, checked between the phases of the read; <= 0 or infinite: none.  Returns 5 when it has passed
   (FreeFormatParserReturnCode::kTimeout -> FilereaderRetcode::kTimeout). */
int pdlp_mi355x_read_mps_timed(const char* path, int32_t num_threads, double time_limit, pdlp_mps_model_t* out);
void pdlp_mi355x_free_mps_model(pdlp_mps_model_t* out);

/* sizeof() of the ABI structs: 0 problem, 1 params, 2 result, 3 iter_stats, 4 prepared, 5 slab_layout, 6 mps_model,
 * 7 task_plan, 8 update; -1 for any other index */
int64_t pdlp_mi355x_sizeof(int32_t which);

const char* pdlp_mi355x_last_error(void);
int pdlp_mi355x_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* PDLP_MI355X_H_ */
