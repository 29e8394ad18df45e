// pdlp_api.cpp — the extern "C" boundary (include/pdlp_mi355x.h).  Exceptions
// never cross it: every entry point catches, records the message for
// pdlp_mi355x_last_error() and returns non-zero (-> HighsStatus::kError).
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <memory>
#include <random>
#include <stdexcept>
#include <string>
#include <thread>
#include <type_traits>
#include <vector>

#include "pdlp_batch.hpp"
#include "pdlp_batch_resident.hpp"
#include "pdlp_halpern.hpp"
#include "pdlp_mps.hpp"
#include "pdlp_pool.hpp"
#include "pdlp_resident.hpp"
#include "pdlp_session.hpp"
#include "pdlp_solver.hpp"
#include "pdlp_update.hpp"
#include "pdlp_detmath.h"

struct pdlp_mi355x_solver {
  pdlp::SolverBase* impl;
};

struct pdlp_mi355x_session {
  pdlp::Session impl;
};

struct pdlp_mi355x_batch {
  std::unique_ptr<pdlp::Batch> impl;
};

namespace {
thread_local std::string g_lastError;

template <typename Fn>
int guarded(Fn&& fn) {
  try {
    fn();
    return 0;
  } catch (const std::exception& e) {
    g_lastError = e.what();
  } catch (...) {
    g_lastError = "unknown exception";
  }
  return 1;
}
}  // namespace

namespace {
template <typename T>
T* dupVec(const std::vector<T>& v) {
  T* p = (T*)malloc(sizeof(T) * (v.size() ? v.size() : 1));
  if (!v.empty()) memcpy(p, v.data(), sizeof(T) * v.size());
  return p;
}
}  // namespace

extern "C" {

const char* pdlp_mi355x_last_error(void) { return g_lastError.c_str(); }
int pdlp_mi355x_abi_version(void) { return PDLP_MI355X_ABI_VERSION; }

void pdlp_mi355x_default_params(pdlp_params_t* opt) {
  if (!opt) return;
  memset(opt, 0, sizeof(*opt));
  opt->primal_tol = 1e-7;  // kDefaultKktTolerance, HConst.h:345
  opt->dual_tol = 1e-7;
  opt->gap_tol = 1e-7;
  opt->time_limit = std::numeric_limits<double>::infinity();
  opt->iter_limit = std::numeric_limits<int32_t>::max();
  opt->features_off = 0;
  opt->restart_method = 1;
  opt->log_level = 0;
  opt->device = 0;
  opt->check_interval = 0;
  opt->algorithm = 0;
  opt->scaling_mode = 5;        // kPdlpScalingRuiz + kPdlpScalingPC (HighsOptions.h:1345-1349)
  opt->ruiz_iterations = 10;    // HighsOptions.h:1353-1355
  opt->step_size_strategy = 1;  // kPdlpStepSizeStrategyAdaptive (HighsOptions.h:1374-1378)
}

int pdlp_mi355x_create(const pdlp_problem_t* P, const pdlp_params_t* opt, pdlp_mi355x_solver_t** out) {
  return pdlp_mi355x_create_sharded(P, opt, 0, 1, nullptr, out);
}

int pdlp_mi355x_create_sharded(const pdlp_problem_t* P, const pdlp_params_t* opt, int32_t rank, int32_t world,
                               const void* id128, pdlp_mi355x_solver_t** out) {
  return guarded([&] {
    if (!P || !opt || !out) throw std::runtime_error("null argument");
    *out = nullptr;
    pdlp::SolverBase* s = nullptr;
    if (opt->algorithm == 1) {
      s = new pdlp::HalpernSolver(*P, *opt, rank, world, id128);
    } else if (opt->algorithm == 0) {
      s = new pdlp::Solver(*P, *opt, rank, world, id128);
    } else {
      throw std::runtime_error("unknown algorithm (0 = cuPDLP-C path, 1 = HiPDLP path)");
    }
    *out = new pdlp_mi355x_solver{s};
  });
}

}  // extern "C"

namespace {
// Devices pdlp_mi355x_solve shards over: opt->num_devices, or PDLP_MI355X_DEVICES when that is 0.
int solveDevices(const pdlp_params_t* opt) {
  int G = opt ? opt->num_devices : 0;
  if (G <= 0) {
    const char* e = getenv("PDLP_MI355X_DEVICES");
    G = e ? atoi(e) : 1;
  }
  return G;
}

// The caller's problem with its 64-bit column starts checked and narrowed into `start` (P.a_start points there).  No HIP
// call happens here, so malformed input gets its own message on a machine without a GPU too.  Every solver path indexes
// the formulated matrix with 32-bit offsets: more than INT32_MAX nonzeros are refused, naming the path that refuses.
struct NarrowedProblem {
  pdlp_problem_t P;
  std::vector<int32_t> start;
};
void narrowProblem(const pdlp_problem_t* P, const int64_t* a_start64, const pdlp_params_t* opt, int devices,
                   NarrowedProblem& out) {
  if (!P || !a_start64 || !opt) throw std::runtime_error("null argument");
  if (P->num_col < 0 || P->num_row < 0) throw std::runtime_error("negative dimensions");
  const int32_t n = P->num_col;
  if (a_start64[0] != 0) throw std::runtime_error("a_start64[0] must be 0, is " + std::to_string(a_start64[0]));
  for (int32_t j = 0; j < n; ++j)
    if (a_start64[j + 1] < a_start64[j])
      throw std::runtime_error("a_start64 decreases at column " + std::to_string(j) + ": a_start64[" + std::to_string(j) +
                               "] = " + std::to_string(a_start64[j]) + ", a_start64[" + std::to_string(j + 1) + "] = " +
                               std::to_string(a_start64[j + 1]));
  if (a_start64[n] != P->num_nz)
    throw std::runtime_error("a_start64[num_col] = " + std::to_string(a_start64[n]) + " differs from num_nz = " +
                             std::to_string(P->num_nz));
  const int64_t kMax = std::numeric_limits<int32_t>::max();
  if (P->num_nz > kMax) {
    const std::string has = "; this problem has " + std::to_string(P->num_nz) + " nonzeros";
    if (opt->algorithm == 1)
      throw std::runtime_error("pdlp_mi355x: the HiPDLP path (algorithm = 1) takes at most INT32_MAX = 2147483647 nonzeros" + has);
    if (devices > 1)
      throw std::runtime_error("pdlp_mi355x: sharded solves (num_devices > 1) take at most INT32_MAX = 2147483647 nonzeros" + has);
    throw std::runtime_error("pdlp_mi355x: the device path indexes the formulated matrix with 32-bit offsets, at most "
                             "INT32_MAX = 2147483647 nonzeros" + has);
  }
  out.P = *P;
  out.start.assign(a_start64, a_start64 + n + 1);  // 0 <= a_start64[j] <= num_nz <= INT32_MAX: exact
  out.P.a_start = out.start.data();
  pdlp::validateProblem(out.P);  // row indices in range, arrays present
}
}  // namespace

extern "C" {

int pdlp_mi355x_create_wide(const pdlp_problem_t* P, const int64_t* a_start64, const pdlp_params_t* opt,
                            pdlp_mi355x_solver_t** out) {
  NarrowedProblem np;
  const int rc = guarded([&] {
    if (!out) throw std::runtime_error("null argument");
    *out = nullptr;
    narrowProblem(P, a_start64, opt, 1, np);
  });
  return rc != 0 ? rc : pdlp_mi355x_create(&np.P, opt, out);
}

int pdlp_mi355x_solve_wide(const pdlp_problem_t* P, const int64_t* a_start64, const pdlp_params_t* opt,
                           pdlp_result_t* R) {
  NarrowedProblem np;
  const int rc = guarded([&] {
    if (!R) throw std::runtime_error("null argument");
    narrowProblem(P, a_start64, opt, solveDevices(opt), np);
  });
  return rc != 0 ? rc : pdlp_mi355x_solve(&np.P, opt, R);
}

int pdlp_mi355x_run(pdlp_mi355x_solver_t* s, pdlp_result_t* R) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("null solver");
    s->impl->run(R);
  });
}

int pdlp_mi355x_update(pdlp_mi355x_solver_t* s, const pdlp_update_t* u) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("pdlp_mi355x_update: null solver");
    if (!u) throw std::runtime_error("pdlp_mi355x_update: null update");
    s->impl->update(*u);
  });
}

int pdlp_mi355x_update_matrix(pdlp_mi355x_solver_t* s, const double* a_value, int64_t num_nz, const pdlp_update_t* u) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("pdlp_mi355x_update_matrix: null solver");
    s->impl->updateMatrix(a_value, num_nz, u);
  });
}

void pdlp_mi355x_destroy(pdlp_mi355x_solver_t* s) {
  if (!s) return;
  try {
    delete s->impl;
  } catch (...) {
  }
  delete s;
}

namespace {
// The multi-GPU form of the one-call boundary: the LP is row-block sharded over G devices of THIS process,
// one host thread per device (each thread owns its device's solver from construction to destruction; the
// ranks meet inside Mesh / Comm exactly as G processes would).  Rank 0 fills the caller's result.
void solveSharded(const pdlp_problem_t& P, const pdlp_params_t& opt, int G, pdlp_result_t* R) {
  int nDev = 0;
  if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0)
    throw std::runtime_error("pdlp_mi355x: no HIP device available (this library has no CPU fallback)");
  // PDLP_MI355X_FOLD_DEVICES=1 (tests on a 1-GPU box): several ranks share a physical device
  const char* f = pdlp::devEnv("PDLP_MI355X_FOLD_DEVICES");
  const bool fold = f && atoi(f) != 0;
  if (!fold && opt.device + G > nDev)
    throw std::runtime_error("pdlp_mi355x: num_devices = " + std::to_string(G) + " starting at device " +
                             std::to_string(opt.device) + ", but only " + std::to_string(nDev) + " HIP devices are visible");
  if (G > 16) throw std::runtime_error("pdlp_mi355x: at most 16 devices");
  unsigned char id[128];
  {
    std::random_device rd;
    for (unsigned char& b : id) b = (unsigned char)rd();
  }
  std::vector<std::string> errors((size_t)G);
  std::vector<pdlp_result_t> scratch((size_t)G);
  // PDLP_MI355X_VERIFY_RANKS=1 (tests): every rank returns its full solution, compared bit for bit below
  const char* vr = pdlp::devEnv("PDLP_MI355X_VERIFY_RANKS");
  const bool verify = vr && atoi(vr) != 0;
  std::vector<std::vector<double>> keep;
  if (verify) keep.resize((size_t)G * 4);
  std::vector<std::thread> workers;
  for (int g = 0; g < G; ++g) {
    workers.emplace_back([&, g] {
      try {
        pdlp_params_t o = opt;
        o.device = fold ? (opt.device + g) % nDev : opt.device + g;
        o.num_devices = 1;
        if (hipSetDevice(o.device) != hipSuccess) throw std::runtime_error("hipSetDevice failed");
        std::unique_ptr<pdlp::SolverBase> s;
        if (o.algorithm == 1) s.reset(new pdlp::HalpernSolver(P, o, g, G, id));
        else if (o.algorithm == 0) s.reset(new pdlp::Solver(P, o, g, G, id));
        else throw std::runtime_error("unknown algorithm (0 = cuPDLP-C path, 1 = HiPDLP path)");
        memset(&scratch[g], 0, sizeof(pdlp_result_t));
        if (verify && g > 0) {
          keep[4 * g + 0].assign((size_t)P.num_col, 0.0); keep[4 * g + 1].assign((size_t)P.num_col, 0.0);
          keep[4 * g + 2].assign((size_t)P.num_row + 1, 0.0); keep[4 * g + 3].assign((size_t)P.num_row + 1, 0.0);
          scratch[g].col_value = keep[4 * g + 0].data(); scratch[g].col_dual = keep[4 * g + 1].data();
          scratch[g].row_value = keep[4 * g + 2].data(); scratch[g].row_dual = keep[4 * g + 3].data();
        }
        s->run(g == 0 ? R : &scratch[g]);
        if (g == 0) scratch[0] = *R;
      } catch (const std::exception& e) {
        errors[g] = e.what()[0] ? e.what() : "error";
      } catch (...) {
        errors[g] = "unknown exception";
      }
    });
  }
  for (std::thread& t : workers) t.join();
  for (int g = 0; g < G; ++g)
    if (!errors[g].empty()) throw std::runtime_error("device rank " + std::to_string(g) + ": " + errors[g]);
  // every rank takes every decision from rank-ordered sums, so they must all report the same bits
  for (int g = 1; g < G; ++g) {
    const pdlp_result_t& a = scratch[0];
    const pdlp_result_t& b = scratch[g];
    bool same = a.term_code == b.term_code && a.num_iter == b.num_iter && a.num_trials == b.num_trials &&
                memcmp(&a.primal_obj, &b.primal_obj, sizeof(double)) == 0 && memcmp(&a.dual_obj, &b.dual_obj, sizeof(double)) == 0;
    if (same && verify && R->col_value && R->row_dual)
      same = memcmp(R->col_value, b.col_value, sizeof(double) * (size_t)P.num_col) == 0 &&
             memcmp(R->row_dual, b.row_dual, sizeof(double) * (size_t)P.num_row) == 0;
    if (!same) throw std::runtime_error("device ranks 0 and " + std::to_string(g) + " disagree (exchange inconsistent)");
  }
}
}  // namespace

int pdlp_mi355x_update_values(pdlp_mi355x_solver_t* s, const double* a_value, int64_t num_nz, const double* q_value, int64_t num_q_nz,
                              const pdlp_update_t* u) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("pdlp_mi355x_update_values: null solver");
    s->impl->updateValues(a_value, num_nz, q_value, num_q_nz, u);
  });
}

int pdlp_mi355x_solve(const pdlp_problem_t* P, const pdlp_params_t* opt, pdlp_result_t* R) {
  const int G = solveDevices(opt);
  if (G > 1) {
    return guarded([&] {
      if (!P || !opt || !R) throw std::runtime_error("null argument");
      solveSharded(*P, *opt, G, R);
    });
  }
  pdlp_mi355x_solver_t* s = nullptr;
  int rc = pdlp_mi355x_create(P, opt, &s);
  if (rc == 0) rc = pdlp_mi355x_run(s, R);
  pdlp_mi355x_destroy(s);
  return rc;
}

int pdlp_mi355x_dims(const pdlp_mi355x_solver_t* s, int32_t* n, int32_t* m, int64_t* nnz, int32_t* nEqs) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("null solver");
    s->impl->dims(n, m, nnz, nEqs);
  });
}

int pdlp_mi355x_reset(pdlp_mi355x_solver_t* s) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("null solver");
    s->impl->reset();
  });
}

int pdlp_mi355x_iterate(pdlp_mi355x_solver_t* s, int32_t n_iters, pdlp_iter_stats_t* st) {
  return guarded([&] {
    if (!s || !s->impl) throw std::runtime_error("null solver");
    s->impl->iterate(n_iters, st);
  });
}

int pdlp_mi355x_get_vector(pdlp_mi355x_solver_t* s, const char* name, double* host, int64_t len) {
  return guarded([&] {
    if (!s || !s->impl || !name || !host) throw std::runtime_error("null argument");
    s->impl->getVector(name, host, len);
  });
}

int pdlp_mi355x_set_vector(pdlp_mi355x_solver_t* s, const char* name, const double* host, int64_t len) {
  return guarded([&] {
    if (!s || !s->impl || !name || !host) throw std::runtime_error("null argument");
    s->impl->setVector(name, host, len);
  });
}

int pdlp_mi355x_stage(pdlp_mi355x_solver_t* s, const char* stage, double* scalars_out, int32_t n_scalars) {
  return guarded([&] {
    if (!s || !s->impl || !stage) throw std::runtime_error("null argument");
    s->impl->stage(stage, scalars_out, n_scalars);
  });
}

int pdlp_mi355x_time_kernel(pdlp_mi355x_solver_t* s, const char* kernel, int32_t reps, double* avg_ms) {
  return guarded([&] {
    if (!s || !s->impl || !kernel || !avg_ms) throw std::runtime_error("null argument");
    *avg_ms = s->impl->timeKernel(kernel, reps);
  });
}

namespace {
// host_prepare, optionally followed by the host restatement of an update (u != nullptr)
void fillPrepared(const pdlp::StandardForm& F, pdlp_prepared_t* out);

void hostPrepare(const pdlp_problem_t* P, const pdlp_params_t* opt, const pdlp_update_t* u, pdlp_prepared_t* out,
                 const double* aValue = nullptr, const pdlp_update_t* uMatrix = nullptr) {
  memset(out, 0, sizeof(*out));
  pdlp::StandardForm F;
  if (opt->algorithm == 1) {  // HiPDLP form: rhs = row lower bounds (row upper bounds are not exported)
    pdlp::formulateHipdlp(*P, F);
    if (!(opt->features_off & PDLP_FEATURE_SCALING_OFF))
      pdlp::scaleHipdlp(F, opt->scaling_mode & 1, opt->scaling_mode & 4, opt->scaling_mode & 2, opt->ruiz_iterations);
  } else {
    pdlp::formulate(*P, F);
    const bool doScale = !(opt->features_off & PDLP_FEATURE_SCALING_OFF);
    F.keepPasses = u != nullptr || aValue != nullptr;
    if (aValue) pdlp::keepUnscaled(F);
    if (doScale) pdlp::scale(F);
    if (aValue) pdlp::hostReplayMatrixUpdate(*P, aValue, uMatrix, doScale, F);
    if (u) pdlp::hostReplayUpdate(*u, F);
  }
  pdlp::finalize(F);
  fillPrepared(F, out);
}

void fillPrepared(const pdlp::StandardForm& F, pdlp_prepared_t* out) {
  out->n = F.n; out->m = F.m; out->n_eqs = F.nEqs; out->n_orig = F.n0; out->nnz = F.nnz;
  out->csr_beg = dupVec(F.csr.beg); out->csr_idx = dupVec(F.csr.idx); out->csr_val = dupVec(F.csr.val);
  out->csc_beg = dupVec(F.cscSorted.beg); out->csc_idx = dupVec(F.cscSorted.idx); out->csc_val = dupVec(F.cscSorted.val);
  out->cost = dupVec(F.cost); out->rhs = dupVec(F.rhs); out->lower = dupVec(F.lower); out->upper = dupVec(F.upper);
  out->col_scale = dupVec(F.colScale); out->row_scale = dupVec(F.rowScale);
  out->row_kind = dupVec(F.rowKind); out->row_new_idx = dupVec(F.rowNewIdx);
  out->norm_cost = F.normCost; out->norm_rhs = F.normRhs; out->mat_norm_inf = F.matNormInf;
  out->spmv_blocks_ax = pdlp::planStream(F.csr.beg, F.m, pdlp::spmvChunkFor(F.nnz), pdlp::kMaxMajorsPerBlock).nBlocks;
  out->spmv_blocks_aty = pdlp::planStream(F.cscSorted.beg, F.n, pdlp::spmvChunkFor(F.nnz), pdlp::kMaxMajorsPerBlock).nBlocks;
}
}  // namespace

int pdlp_mi355x_host_prepare(const pdlp_problem_t* P, const pdlp_params_t* opt, pdlp_prepared_t* out) {
  return guarded([&] {
    if (!P || !opt || !out) throw std::runtime_error("null argument");
    hostPrepare(P, opt, nullptr, out);
  });
}

int pdlp_mi355x_host_prepare_updated(const pdlp_problem_t* P, const pdlp_params_t* opt, const pdlp_update_t* u,
                                     pdlp_prepared_t* out) {
  return guarded([&] {
    if (!P || !opt || !out) throw std::runtime_error("null argument");
    if (!u) throw std::runtime_error("pdlp_mi355x_update: null update");
    // the refusals of pdlp_mi355x_update that depend on how the solver was created
    if (opt->algorithm == 1) pdlp::refuseHipdlp(pdlp::kEntryUpdate);
    if (!opt->updatable) pdlp::refuseNotUpdatable(pdlp::kEntryUpdate);
    hostPrepare(P, opt, u, out);
  });
}

// Test hook, not part of the public header: the entry below with a pdlp_mi355x_update (u_then, may be NULL) applied to
// the result on the same form — what shows that a data update after a matrix update replays the NEW factors.
int pdlp_mi355x_host_prepare_updated_matrix_then(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value,
                                                 const pdlp_update_t* u, const pdlp_update_t* u_then, pdlp_prepared_t* out) {
  return guarded([&] {
    if (!P || !opt || !out) throw std::runtime_error("null argument");
    // the refusals of pdlp_mi355x_update_matrix that depend on how the solver was created
    if (opt->algorithm == 1) pdlp::refuseHipdlp(pdlp::kEntryUpdateMatrix);
    if (!(opt->updatable & PDLP_UPDATABLE_MATRIX)) pdlp::refuseNoMatrixBit(pdlp::kEntryUpdateMatrix);
    if (pdlp::hessianHasOffDiagonal(*P)) pdlp::refuseOffDiagonalHessian(pdlp::kEntryUpdateMatrix);
    if (!a_value) throw std::runtime_error("pdlp_mi355x_update_matrix: a_value is NULL");
    hostPrepare(P, opt, u_then, out, a_value, u);
  });
}

int pdlp_mi355x_host_prepare_updated_matrix(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value,
                                            const pdlp_update_t* u, pdlp_prepared_t* out) {
  return pdlp_mi355x_host_prepare_updated_matrix_then(P, opt, a_value, u, nullptr, out);
}

// Host twin of create with the pattern contract of PDLP_UPDATABLE_HESSIAN and of pdlp_mi355x_update_values; u_then (test
// hook, may be NULL): a pdlp_mi355x_update applied to the result on the same form.
int pdlp_mi355x_host_prepare_qp_then(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value, const double* q_value,
                                     const pdlp_update_t* u, const pdlp_update_t* u_then, pdlp_prepared_t* out,
                                     pdlp_prepared_hessian_t* qout) {
  return guarded([&] {
    if (!P || !opt || !out || !qout) throw std::runtime_error("null argument");
    memset(out, 0, sizeof(*out));
    memset(qout, 0, sizeof(*qout));
    const bool change = a_value || q_value || u || u_then;
    const bool keepQ = (opt->updatable & PDLP_UPDATABLE_HESSIAN) != 0;
    if (change) {  // the refusals of pdlp_mi355x_update_values that depend on how the solver was created
      if (opt->algorithm == 1) pdlp::refuseHipdlp(pdlp::kEntryUpdateValues);
      if (!keepQ) pdlp::refuseNoHessianBit(pdlp::kEntryUpdateValues);
      if (a_value && !(opt->updatable & PDLP_UPDATABLE_MATRIX)) pdlp::refuseNoMatrixBit(pdlp::kEntryUpdateValues);
    }
    if (opt->algorithm == 1) throw std::runtime_error("pdlp_mi355x_host_prepare_qp: the cuPDLP-C form only (algorithm = 0)");
    pdlp::StandardForm F;
    pdlp::formulate(*P, F, keepQ);
    const bool doScale = !(opt->features_off & PDLP_FEATURE_SCALING_OFF);
    F.keepPasses = change;
    if (change) {
      if (opt->updatable & PDLP_UPDATABLE_MATRIX) pdlp::keepUnscaled(F);
      pdlp::keepUnscaledHessian(F);
    }
    if (doScale) pdlp::scale(F);
    if (change) {
      if (q_value) pdlp::checkHessianUpdateShape(q_value, F.hmap.nSlots, F.hmap.kept(), F.hmap.nSlots);
      if (a_value) {
        pdlp::hostReplayMatrixUpdate(*P, a_value, u, doScale, F, q_value);
      } else {
        static const pdlp_update_t kNoData{};
        const pdlp_update_t& ud = u ? *u : kNoData;
        pdlp::checkUpdateShape(ud);
        if (pdlp::updateMask(ud) & pdlp::kUpdRows) pdlp::refuseKindChange(F.rowKind.data(), F.m, ud.row_lower, ud.row_upper);
        if (q_value) pdlp::hostReplayHessianUpdate(q_value, F);  // (validates before it writes; u has been validated above)
        pdlp::hostReplayUpdate(ud, F);
      }
      if (u_then) pdlp::hostReplayUpdate(*u_then, F);
    }
    pdlp::finalize(F);
    fillPrepared(F, out);
    qout->n = F.n;
    qout->has_diag = F.qdiag.empty() ? 0 : 1;
    qout->nnz_off = F.qoff.beg.empty() ? 0 : (int64_t)F.qoff.beg[F.n];
    qout->qdiag = dupVec(F.qdiag);
    qout->q_beg = dupVec(F.qoff.beg); qout->q_idx = dupVec(F.qoff.idx); qout->q_val = dupVec(F.qoff.val);
  });
}

int pdlp_mi355x_host_prepare_qp(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value, const double* q_value,
                                const pdlp_update_t* u, pdlp_prepared_t* out, pdlp_prepared_hessian_t* qout) {
  return pdlp_mi355x_host_prepare_qp_then(P, opt, a_value, q_value, u, nullptr, out, qout);
}

void pdlp_mi355x_free_prepared_hessian(pdlp_prepared_hessian_t* o) {
  if (!o) return;
  free(o->qdiag); free(o->q_beg); free(o->q_idx); free(o->q_val);
  memset(o, 0, sizeof(*o));
}

void pdlp_mi355x_free_prepared(pdlp_prepared_t* o) {
  if (!o) return;
  free(o->csr_beg); free(o->csr_idx); free(o->csr_val); free(o->csc_beg); free(o->csc_idx); free(o->csc_val);
  free(o->cost); free(o->rhs); free(o->lower); free(o->upper); free(o->col_scale); free(o->row_scale);
  free(o->row_kind); free(o->row_new_idx);
  memset(o, 0, sizeof(*o));
}

int pdlp_mi355x_row_partition(const pdlp_prepared_t* prep, int32_t world, int32_t* offsets) {
  return guarded([&] {
    if (!prep || !offsets || world < 1) throw std::runtime_error("bad argument");
    pdlp::Compressed csr;
    csr.beg.assign(prep->csr_beg, prep->csr_beg + prep->m + 1);
    std::vector<int32_t> off = pdlp::rowPartition(csr, prep->m, world);
    for (int32_t g = 0; g <= world; ++g) offsets[g] = off[g];
  });
}

int pdlp_mi355x_host_slab_layout(const pdlp_prepared_t* prep, int32_t which, int32_t long_limit,
                                 pdlp_slab_layout_t* out) {
  return guarded([&] {
    if (!prep || !out) throw std::runtime_error("null argument");
    memset(out, 0, sizeof(*out));
    const int32_t nMajor = which ? prep->n : prep->m, nMinor = which ? prep->m : prep->n;
    pdlp::Compressed c;
    const int32_t* beg = which ? prep->csc_beg : prep->csr_beg;
    c.beg.assign(beg, beg + nMajor + 1);
    c.idx.assign(which ? prep->csc_idx : prep->csr_idx, (which ? prep->csc_idx : prep->csr_idx) + prep->nnz);
    c.val.assign(which ? prep->csc_val : prep->csr_val, (which ? prep->csc_val : prep->csr_val) + prep->nnz);
    pdlp::SlabLayout L;
    pdlp::buildSlabLayout(c, nMajor, nMinor, long_limit, pdlp::kSlabWidthLog2, which ? pdlp::kSlabMajorCostCols : pdlp::kSlabMajorCostRows, L);
    out->rows_per_block = L.rowsPerBlock; out->rows_per_wave = 0; out->n_blocks = L.nBlocks;
    out->minor_bits = L.minorBits; out->slab_width_log2 = L.slabWidthLog2;
    out->n_long = (int32_t)L.longMap.size(); out->nnz_short = (int64_t)L.ent.size();
    out->wave_ptr = dupVec(L.wavePtr); out->ent = dupVec(L.ent); out->val = dupVec(L.val);
    out->long_mask = dupVec(L.longMask); out->long_map = dupVec(L.longMap); out->wave_beg = dupVec(L.waveBeg);
  });
}

void pdlp_mi355x_free_slab_layout(pdlp_slab_layout_t* o) {
  if (!o) return;
  free(o->wave_ptr); free(o->ent); free(o->val); free(o->long_mask); free(o->long_map); free(o->wave_beg);
  memset(o, 0, sizeof(*o));
}

int pdlp_mi355x_host_task_plan(const pdlp_prepared_t* prep, int32_t which, int32_t long_limit, int32_t balance,
                               pdlp_task_plan_t* out) {
  return guarded([&] {
    if (!prep || !out) throw std::runtime_error("null argument");
    memset(out, 0, sizeof(*out));
    const int32_t nMajor = which ? prep->n : prep->m, nMinor = which ? prep->m : prep->n;
    pdlp::Compressed c;
    const int32_t* beg = which ? prep->csc_beg : prep->csr_beg;
    c.beg.assign(beg, beg + nMajor + 1);
    c.idx.assign(which ? prep->csc_idx : prep->csr_idx, (which ? prep->csc_idx : prep->csr_idx) + prep->nnz);
    c.val.assign(which ? prep->csc_val : prep->csr_val, (which ? prep->csc_val : prep->csr_val) + prep->nnz);
    const int32_t majorCost = which ? pdlp::kSlabMajorCostCols : pdlp::kSlabMajorCostRows;
    // the same calls, in the same order, as DeviceMatrix::upload (pdlp_solver.cpp)
    std::vector<int32_t> cold((size_t)std::max(nMajor, 1));
    pdlp::slabColdCounts(c.beg.data(), c.idx.data(), nMajor, nMinor, long_limit, cold.data());
    const pdlp::SlabPartition part = pdlp::slabPartition(c.beg.data(), cold.data(), nMajor, nMinor, long_limit, majorCost);
    std::vector<int32_t> lo, hi, cnt;
    const int32_t tileLog2 = pdlp::xcdTileLog2(nMinor), nTiles = pdlp::xcdTileCount(nMinor, tileLog2);
    const std::vector<int32_t> hist = pdlp::slabTileHistogram(c.beg.data(), c.idx.data(), part, long_limit, tileLog2, nTiles, lo, hi, cnt);
    const std::vector<int8_t> owner = pdlp::xcdTileOwners(hist, nTiles);
    pdlp::SlabLayout L;
    pdlp::buildSlabLayout(c, nMajor, nMinor, long_limit, pdlp::kSlabWidthLog2, majorCost, L);
    int32_t taskGroup = 0;
    const int32_t nLong = (int32_t)L.longMap.size();
    const pdlp::LongPlan P = pdlp::planSlabTasks(L.longCsr.beg, L.longCsr.idx.data(), nLong, L.longMap.data(), balance != 0, &owner, tileLog2,
                                                 L.nBlocks, taskGroup);
    out->n_tasks = P.nTasks; out->task_group = taskGroup; out->n_seg_slots = P.nSegSlots; out->n_long = nLong;
    out->n_blocks = L.nBlocks; out->tile_log2 = tileLog2; out->n_tiles = nTiles;
    std::vector<int32_t> flat((size_t)8 * P.nTasks);
    if (P.nTasks > 0) memcpy(flat.data(), P.tasks.data(), flat.size() * sizeof(int32_t));
    out->tasks = dupVec(flat); out->tile_owner = dupVec(owner); out->long_beg = dupVec(L.longCsr.beg); out->long_idx = dupVec(L.longCsr.idx);
  });
}

void pdlp_mi355x_free_task_plan(pdlp_task_plan_t* o) {
  if (!o) return;
  free(o->tasks); free(o->tile_owner); free(o->long_beg); free(o->long_idx);
  memset(o, 0, sizeof(*o));
}

// TEST HOOK, not part of the public header (no product code calls it): the work plan of operand `which` (0: A by rows,
// 1: A' by columns), for the CPU tests of the structural thresholds.  slab_long_limit = 0, the stream layout: planStream and
// planLong, the same calls as in DeviceMatrix::uploadPlans — work blocks of whole short majors (block_beg: first major, end
// major, first entry, end entry), the majors beyond the chunk and their segment tasks in workgroups of task_group (records
// as in pdlp_task_plan_t).  slab_long_limit > 0 (as in pdlp_mi355x_host_slab_layout): this branch only COUNTS the slab
// layout's long majors, from a layout of the default slab width — it does not plan their tasks as uploadPlans does
// (planSlabTasks: pdlp_mi355x_host_task_plan shows those).  long_group: long majors per contribution slot (longGroupFor, as
// uploadPlans).  small_grid: workgroups the persistent trial loop asks for where both operands qualify (smallGridFor over the
// blocks of A and A'; extra_blocks: those of a third operand, 0 for none).
struct pdlp_stream_plan_t {
  int32_t chunk, n_blocks, n_long, n_tasks, task_group, long_group, long_slots, small_grid;
  int32_t *block_beg, *long_majors, *tasks;  // [4*n_blocks], [n_long], [8*n_tasks]
};
int pdlp_mi355x_host_stream_plan(const pdlp_prepared_t* prep, int32_t which, int32_t slab_long_limit, int32_t extra_blocks,
                                 pdlp_stream_plan_t* out) {
  return guarded([&] {
    if (!prep || !out) throw std::runtime_error("null argument");
    memset(out, 0, sizeof(*out));
    const int32_t nMajor = which ? prep->n : prep->m, nMinor = which ? prep->m : prep->n;
    const int32_t* beg = which ? prep->csc_beg : prep->csr_beg;
    const std::vector<int32_t> hostBeg(beg, beg + nMajor + 1);
    const int32_t blocks = std::max(std::max(prep->spmv_blocks_ax, prep->spmv_blocks_aty), extra_blocks);
    out->small_grid = pdlp::smallGridFor(blocks, prep->n);
    if (slab_long_limit > 0) {
      pdlp::Compressed c;
      c.beg = hostBeg;
      c.idx.assign(which ? prep->csc_idx : prep->csr_idx, (which ? prep->csc_idx : prep->csr_idx) + prep->nnz);
      c.val.assign(which ? prep->csc_val : prep->csr_val, (which ? prep->csc_val : prep->csr_val) + prep->nnz);
      pdlp::SlabLayout L;
      pdlp::buildSlabLayout(c, nMajor, nMinor, slab_long_limit, pdlp::kSlabWidthLog2, which ? pdlp::kSlabMajorCostCols : pdlp::kSlabMajorCostRows, L);
      out->chunk = slab_long_limit;
      out->n_long = (int32_t)L.longMap.size();
      out->long_majors = dupVec(L.longMap);
    } else {
      out->chunk = pdlp::spmvChunkFor(hostBeg[nMajor]);
      const pdlp::StreamPlan plan = pdlp::planStream(hostBeg, nMajor, out->chunk, pdlp::kMaxMajorsPerBlock);
      out->task_group = pdlp::kSpmvThreads / 64;
      const pdlp::LongPlan L = pdlp::planLong(hostBeg, plan.longMajors, nullptr, out->task_group);
      out->n_blocks = plan.nBlocks;
      out->n_long = L.nLong;
      out->n_tasks = L.nTasks;
      std::vector<int32_t> flat((size_t)8 * L.nTasks);
      if (L.nTasks > 0) memcpy(flat.data(), L.tasks.data(), flat.size() * sizeof(int32_t));
      out->block_beg = dupVec(plan.blockBeg); out->long_majors = dupVec(plan.longMajors); out->tasks = dupVec(flat);
    }
    out->long_group = pdlp::longGroupFor(out->n_long);
    out->long_slots = (out->n_long + out->long_group - 1) / out->long_group;
  });
}
void pdlp_mi355x_free_stream_plan(pdlp_stream_plan_t* o) {
  if (!o) return;
  free(o->block_beg); free(o->long_majors); free(o->tasks);
  memset(o, 0, sizeof(*o));
}

// TEST HOOK, not part of the public header: the rule that decides whether a HiPDLP solver runs the steps 2..40 of a block as
// one persistent launch (pdlp_halpern_small.hpp halpernSmallReason — the function HalpernSolver calls), on shapes given by
// hand.  shape[11]: blocks of A, blocks of A', chunk of A, chunk of A', use_slab, long-major tasks, long-major contribution
// groups, sharded, profile mode, switch on, resident workgroups.  *reason: 0 persistent, else why not; *grid: the launch's
// working workgroups; *mode: 1 XCD-local, 0 agent scope (meaningful where *reason is 0).
int pdlp_mi355x_host_hipdlp_small_rule(const int32_t* shape, int32_t xcd_local_allowed, int32_t* reason, int32_t* grid, int32_t* mode) {
  return guarded([&] {
    if (!shape || !reason || !grid || !mode) throw std::runtime_error("null argument");
    pdlp::HalpernSmallShape s{};
    s.blocksA = shape[0]; s.blocksAt = shape[1]; s.chunkA = shape[2]; s.chunkAt = shape[3]; s.useSlab = shape[4];
    s.longTasks = shape[5]; s.longContrib = shape[6]; s.sharded = shape[7]; s.profile = shape[8]; s.switchOn = shape[9];
    s.resident = shape[10];
    *reason = pdlp::halpernSmallReason(s);
    *grid = pdlp::halpernSmallGrid(s);
    *mode = pdlp::halpernSmallMode(*grid, xcd_local_allowed != 0);
  });
}

// TEST HOOK, not part of the public header: the rule that decides where a QP's Hessian is extracted (pdlp_setup.hpp
// hessianExtractionReason — the function gpuPrepare and the solver call), on facts given by hand.  q_start: q_dim + 1
// entries, or NULL.  *reason: 0 on the device, else why the host walk runs (the codes of stage "hessian_extraction").
int pdlp_mi355x_host_hessian_extraction_rule(int32_t gpu_setup, int32_t sharded, int32_t hipdlp, int32_t switch_on, int32_t q_dim,
                                             const int32_t* q_start, int32_t* reason) {
  return guarded([&] {
    if (!reason) throw std::runtime_error("null argument");
    *reason = pdlp::hessianExtractionReason(gpu_setup != 0, sharded != 0, hipdlp != 0, switch_on != 0, q_dim, q_start);
  });
}

// TEST HOOK, not part of the public header (no product code calls it): what a solver holds of operand `which` (0: A by rows,
// 1: A' by columns) after its set-up, on the host or on the device — downloaded as it lies in HBM, with no launch and no
// change of state.  Stream layout (use_slab = 0): beg / idx / val are the operand's CSR, block_beg its work blocks
// [4 * n_blocks].  Slab layout: beg / idx / val are the compact CSR of the long majors (long_map: compact index -> major),
// wave_beg / wave_ptr [16 * slab_blocks + 1], ent / slab_val [nnz_short], long_mask [n_mask_words], and what the build
// decided on the way: tile_owner [n_tiles], span_lo / span_hi / span_cnt [slab_blocks].  idx / val / ent / slab_val come
// with their pad element (nnz_csr + 1, nnz_short + 1 entries).  tasks: [8 * n_tasks], records as in pdlp_task_plan_t.
struct pdlp_device_matrix_t {
  int32_t use_slab, n_major, n_minor, chunk, n_blocks, slab_blocks, rows_per_block, minor_bits;
  int32_t slab_width_log2, n_long, n_tasks, task_group, long_group, long_slots, tile_log2, n_tiles;
  int32_t n_mask_words, n_csr_major;
  int64_t nnz, nnz_short, nnz_csr;
  int32_t *beg, *idx, *block_beg, *wave_beg, *wave_ptr, *long_map, *tasks, *span_lo, *span_hi, *span_cnt;
  uint32_t *ent, *long_mask;
  double *val, *slab_val;
  int8_t* tile_owner;
};
int pdlp_mi355x_device_matrix(pdlp_mi355x_solver_t* h, int32_t which, pdlp_device_matrix_t* out) {
  return guarded([&] {
    if (!h || !h->impl || !out) throw std::runtime_error("null argument");
    if (which != 0 && which != 1) throw std::runtime_error("pdlp_mi355x_device_matrix: which is 0 (A) or 1 (A')");
    memset(out, 0, sizeof(*out));
    hipStream_t s = nullptr;
    const pdlp::DeviceMatrix& M = *h->impl->deviceMatrix(which, &s);
    out->use_slab = M.useSlab ? 1 : 0; out->n_major = M.nMajor; out->n_minor = M.nMinor; out->chunk = M.chunk;
    out->n_blocks = M.nBlocks; out->n_long = M.nLong; out->n_tasks = M.nTasks; out->task_group = M.taskGroup;
    out->long_group = M.longGroup; out->long_slots = M.longSlots; out->nnz = M.nnz;
    out->n_csr_major = M.beg.size() ? (int32_t)M.beg.size() - 1 : 0;
    auto pull = [&](const auto& dev, size_t count) {
      using T = typename std::remove_pointer<decltype(dev.get())>::type;
      if (count > dev.size()) throw std::runtime_error("pdlp_mi355x_device_matrix: an array is shorter than its layout says");
      std::vector<T> v(count);
      dev.download(v.data(), count, s);
      PDLP_HIP(hipStreamSynchronize(s));
      return v;
    };
    const std::vector<int32_t> beg = pull(M.beg, M.beg.size());
    out->nnz_csr = beg.empty() ? 0 : beg.back();
    out->beg = dupVec(beg);
    out->idx = dupVec(pull(M.idx, (size_t)out->nnz_csr + 1));
    out->val = dupVec(pull(M.val, (size_t)out->nnz_csr + 1));
    out->block_beg = dupVec(pull(M.blockBeg, (size_t)4 * M.nBlocks));
    static_assert(sizeof(pdlp::LongTask) == 8 * sizeof(int32_t), "task record layout");
    {
      const std::vector<pdlp::LongTask> t = pull(M.lTasks, (size_t)M.nTasks);
      std::vector<int32_t> flat((size_t)8 * M.nTasks);
      if (M.nTasks > 0) memcpy(flat.data(), t.data(), flat.size() * sizeof(int32_t));
      out->tasks = dupVec(flat);
    }
    if (M.useSlab) {
      const int32_t nB = M.slab.nBlocks;
      out->slab_blocks = nB; out->rows_per_block = M.slab.rowsPerBlock; out->minor_bits = M.slab.minorBits;
      out->slab_width_log2 = M.slabWidthLog2; out->tile_log2 = M.tileLog2; out->n_tiles = (int32_t)M.hostTileOwner.size();
      out->n_mask_words = (int32_t)M.longMask.size();
      const std::vector<int32_t> wavePtr = pull(M.wavePtr, (size_t)nB * pdlp::kSlabWavesPerBlock + 1);
      out->nnz_short = wavePtr.back();
      out->wave_ptr = dupVec(wavePtr);
      out->wave_beg = dupVec(pull(M.waveBeg, (size_t)nB * pdlp::kSlabWavesPerBlock + 1));
      out->ent = dupVec(pull(M.ent, (size_t)out->nnz_short + 1));
      out->slab_val = dupVec(pull(M.slabVal, (size_t)out->nnz_short + 1));
      out->long_mask = dupVec(pull(M.longMask, M.longMask.size()));
      out->long_map = dupVec(M.hostLongMap);
      out->tile_owner = dupVec(M.hostTileOwner);
      out->span_lo = dupVec(M.hostSpanLo); out->span_hi = dupVec(M.hostSpanHi); out->span_cnt = dupVec(M.hostSpanCnt);
    }
  });
}
void pdlp_mi355x_free_device_matrix(pdlp_device_matrix_t* o) {
  if (!o) return;
  free(o->beg); free(o->idx); free(o->block_beg); free(o->wave_beg); free(o->wave_ptr); free(o->long_map); free(o->tasks);
  free(o->span_lo); free(o->span_hi); free(o->span_cnt); free(o->ent); free(o->long_mask); free(o->val); free(o->slab_val);
  free(o->tile_owner);
  memset(o, 0, sizeof(*o));
}

void pdlp_mi355x_det_exp_log(int32_t n, const double* x, double* exp_out, double* log_out) {
  for (int32_t i = 0; i < n; ++i) { exp_out[i] = pdlp_det_exp(x[i]); log_out[i] = pdlp_det_log(x[i]); }
}

int64_t pdlp_mi355x_sizeof(int32_t which) {
  switch (which) {
    case 0: return sizeof(pdlp_problem_t);
    case 1: return sizeof(pdlp_params_t);
    case 2: return sizeof(pdlp_result_t);
    case 3: return sizeof(pdlp_iter_stats_t);
    case 4: return sizeof(pdlp_prepared_t);
    case 5: return sizeof(pdlp_slab_layout_t);
    case 6: return sizeof(pdlp_mps_model_t);
    case 7: return sizeof(pdlp_task_plan_t);
    case 8: return sizeof(pdlp_update_t);
    default: return -1;
  }
}

// ---- sessions (pdlp_session.hpp) --------------------------------------------------------------------------------------
int pdlp_mi355x_session_create(pdlp_mi355x_session_t** out) {
  return guarded([&] {
    if (!out) throw std::runtime_error("pdlp_mi355x_session_create: null argument");
    *out = new pdlp_mi355x_session();  // (no HIP call: a session holds nothing until its first solve)
  });
}

int pdlp_mi355x_session_solve(pdlp_mi355x_session_t* S, const pdlp_problem_t* P, const pdlp_params_t* opt, pdlp_result_t* R) {
  int rc = 0;
  const int thrown = guarded([&] {
    if (!S) throw std::runtime_error("pdlp_mi355x_session_solve: null session");
    if (!P || !opt || !R) throw std::runtime_error("null argument");
    rc = S->impl.solve(*P, *opt, R);
  });
  return thrown ? thrown : rc;
}

int pdlp_mi355x_session_info(const pdlp_mi355x_session_t* S, pdlp_session_info_t* out) {
  return guarded([&] {
    if (!S || !out) throw std::runtime_error("pdlp_mi355x_session_info: null argument");
    *out = S->impl.info();
  });
}

void pdlp_mi355x_session_release(pdlp_mi355x_session_t* S) {
  if (S) S->impl.release();
}

void pdlp_mi355x_session_destroy(pdlp_mi355x_session_t* S) {
  if (!S) return;
  S->impl.release();
  delete S;
}

int64_t pdlp_mi355x_session_info_size(void) { return sizeof(pdlp_session_info_t); }

// ---- batches (pdlp_batch.hpp) -------------------------------------------------------------------------------------------
int pdlp_mi355x_batch_create(const pdlp_problem_t* P, const pdlp_params_t* opt, int32_t lanes, pdlp_mi355x_batch_t** out) {
  return guarded([&] {
    if (!P || !opt || !out) throw std::runtime_error("pdlp_mi355x_batch_create: null argument");
    *out = nullptr;
    std::unique_ptr<pdlp::Batch> b(new pdlp::Batch(*P, *opt, lanes));  // (the refusals by name come before any HIP call)
    *out = new pdlp_mi355x_batch{std::move(b)};
  });
}

int pdlp_mi355x_batch_run(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_update_t* u, pdlp_result_t* R) {
  return guarded([&] {
    if (!B || !B->impl) throw std::runtime_error("pdlp_mi355x_batch_run: null batch");
    B->impl->run(K, u, R);
  });
}

int pdlp_mi355x_batch_run_values(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_variant_t* v, pdlp_result_t* R) {
  return guarded([&] {
    if (!B || !B->impl) throw std::runtime_error("pdlp_mi355x_batch_run_values: null batch");
    B->impl->runValues(K, v, R);
  });
}

int64_t pdlp_mi355x_variant_size(void) { return sizeof(pdlp_variant_t); }

// Test hook, not part of the public header: what pdlp_mi355x_batch_run_values refuses, for a batch created on P with opt,
// before it looks at a matrix or Hessian value — no device call is made.
int pdlp_mi355x_host_batch_variants_refusal(const pdlp_problem_t* P, const pdlp_params_t* opt, int32_t K, const pdlp_variant_t* v,
                                            const pdlp_result_t* R) {
  return guarded([&] {
    if (!P || !opt) throw std::runtime_error("null argument");
    pdlp::refuseBatchArguments(pdlp::kEntryBatchRunValues, K, v, R);
    for (int32_t k = 0; k < K; ++k) {
      const std::string why = pdlp::batchVariantRefusal(*P, *opt, v[k]);
      if (!why.empty()) throw std::runtime_error("variant " + std::to_string(k) + ": " + why);
    }
  });
}

// Variants and solutions as arrays already in HBM on the batch's device (pdlp_batch_resident.hpp).  The refusals that need
// no device come first, the arguments' before the handle's.
int pdlp_mi355x_batch_run_device(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_variant_t* v_dev, pdlp_result_t* R_dev, void* stream) {
  return guarded([&] {
    pdlp::refuseBatchArguments(pdlp::kEntryBatchRunDevice, K, v_dev, R_dev);
    if (!B || !B->impl) throw std::runtime_error("pdlp_mi355x_batch_run_device: null batch");
    B->impl->runDevice(K, v_dev, R_dev, (hipStream_t)stream);
  });
}

// Test hook, not part of the public header: refusal step 1 of pdlp_mi355x_batch_run_device, for a batch created on P with
// opt — from the pointers' being NULL or not alone; no array of a variant is read, no device call is made.
int pdlp_mi355x_host_batch_device_variants_refusal(const pdlp_problem_t* P, const pdlp_params_t* opt, int32_t K,
                                                   const pdlp_variant_t* v, const pdlp_result_t* R) {
  return guarded([&] {
    if (!P || !opt) throw std::runtime_error("null argument");
    pdlp::refuseBatchArguments(pdlp::kEntryBatchRunDevice, K, v, R);
    for (int32_t k = 0; k < K; ++k) {
      const std::string why = pdlp::batchVariantDeviceRefusal(*P, *opt, v[k]);
      if (!why.empty()) throw std::runtime_error("variant " + std::to_string(k) + ": " + why);
    }
  });
}

// Test hook, not part of the public header: refusal step 3's verdict on canned records (three int32 per variant:
// firstBadRow, anyNonzero, firstNegDiag) — what pdlp_mi355x_batch_run_device makes of the validation launch's output.  The
// arrays of v are HOST arrays here: they are asked whether they are NULL, and the named row's two bounds are read.
int pdlp_mi355x_host_batch_records_verdict(int32_t K, const pdlp_variant_t* v, const int32_t* records, const int32_t* row_kind,
                                           int32_t m, int32_t n) {
  return guarded([&] {
    if (K < 1 || !v || !records || (m > 0 && !row_kind)) throw std::runtime_error("null argument");
    static_assert(sizeof(pdlp::VariantRecord) == 3 * sizeof(int32_t), "three int32 per record");
    pdlp::refuseByRecords(K, v, reinterpret_cast<const pdlp::VariantRecord*>(records), row_kind, m, n,
                          [&](int32_t k, int32_t row, double* lo, double* up) {
                            *lo = v[k].u.row_lower[row];
                            *up = v[k].u.row_upper[row];
                          });
  });
}

// Test hook, not part of the public header and NOT ABI — unsupported, it may change or go without an ABI version step: the
// validation launch alone.  Unlike the host-only hooks above it works on a live batch and on the device: it runs step 1 and
// the pointer check on v_dev first (so no host pointer reaches the kernel), then initialises n_rec >= K records, launches
// the K jobs and writes all n_rec records, three int32 each, to out — out must hold 3 * n_rec int32; K < 1, a null
// argument and n_rec < K are refused.  Nothing of a lane is written.
int pdlp_mi355x_batch_variant_records(pdlp_mi355x_batch_t* B, int32_t K, const pdlp_variant_t* v_dev, int32_t n_rec, int32_t* out) {
  return guarded([&] {
    if (!B || !B->impl) throw std::runtime_error("pdlp_mi355x_batch_variant_records: null batch");
    B->impl->variantRecords(K, v_dev, n_rec, out);
  });
}

int pdlp_mi355x_batch_info(const pdlp_mi355x_batch_t* B, pdlp_batch_info_t* out) {
  return guarded([&] {
    if (!B || !B->impl || !out) throw std::runtime_error("pdlp_mi355x_batch_info: null argument");
    *out = B->impl->info();
  });
}

void pdlp_mi355x_batch_destroy(pdlp_mi355x_batch_t* B) {
  if (!B) return;
  try {
    B->impl.reset();
  } catch (...) {
  }
  delete B;
}

int64_t pdlp_mi355x_batch_info_size(void) { return sizeof(pdlp_batch_info_t); }

// ---- device-resident entries (pdlp_resident.hpp) -------------------------------------------------------------------------
}  // extern "C"
namespace {
// guarded(), with the entry's name in front of whatever is refused
template <typename Fn>
int guardedAs(const char* entry, Fn&& fn) {
  return guarded([&] {
    try {
      fn();
    } catch (const std::exception& e) {
      throw std::runtime_error(std::string(entry) + ": " + e.what());
    }
  });
}
}  // namespace
extern "C" {

int pdlp_mi355x_create_device(const pdlp_problem_t* P_dev, const pdlp_params_t* opt, void* stream, pdlp_mi355x_solver_t** out) {
  return guardedAs(pdlp::kEntryCreateDevice, [&] {
    if (!P_dev || !opt || !out) throw std::runtime_error("null argument");
    *out = nullptr;
    // what needs no device comes before any HIP call
    if (opt->algorithm != 0 && opt->algorithm != 1) throw std::runtime_error("unknown algorithm (0 = cuPDLP-C path, 1 = HiPDLP path)");
    if (const char* why = pdlp::sessionOneShotReason(*opt)) throw std::runtime_error(why);
    pdlp::residentProblemShape(*P_dev);
    int nDev = 0;
    if (hipGetDeviceCount(&nDev) != hipSuccess || nDev <= 0)
      throw std::runtime_error("pdlp_mi355x: no HIP device available (this library has no CPU fallback)");
    pdlp::requireDeviceProblem(*P_dev, opt->device);
    pdlp::ResidentProblem RP(*P_dev, (hipStream_t)stream);
    *out = new pdlp_mi355x_solver{new pdlp::Solver(RP, *opt)};
  });
}

int pdlp_mi355x_update_device(pdlp_mi355x_solver_t* s, const double* a_value_dev, int64_t num_nz, const double* q_value_dev,
                              int64_t num_q_nz, const pdlp_update_t* u_dev, void* stream) {
  return guardedAs(pdlp::kEntryUpdateDevice, [&] {
    if (!s || !s->impl) throw std::runtime_error("null solver");
    s->impl->updateDevice(a_value_dev, num_nz, q_value_dev, num_q_nz, u_dev, (hipStream_t)stream);
  });
}

int pdlp_mi355x_run_device(pdlp_mi355x_solver_t* s, pdlp_result_t* R_dev) {
  return guardedAs(pdlp::kEntryRunDevice, [&] {
    if (!s || !s->impl) throw std::runtime_error("null solver");
    s->impl->runDevice(R_dev);
  });
}

// Test hook, not part of the public header: what pdlp_mi355x_update_device refuses before any HIP call, for a solver created
// on P with opt — from the pointers' being NULL or not alone; no array of the update is read, no device call is made.
int pdlp_mi355x_host_update_device_refusal(const pdlp_problem_t* P, const pdlp_params_t* opt, const double* a_value, int64_t num_nz,
                                           const double* q_value, int64_t num_q_nz, const pdlp_update_t* u) {
  return guardedAs(pdlp::kEntryUpdateDevice, [&] {
    if (!P || !opt) throw std::runtime_error("null argument");
    if (const char* why = pdlp::sessionOneShotReason(*opt)) throw std::runtime_error(why);
    pdlp::ValueUpdateFacts f;
    f.updatable = opt->updatable;
    f.nnz = P->num_col > 0 && P->a_start ? (int64_t)P->a_start[P->num_col] : 0;
    f.qSlots = (opt->updatable & PDLP_UPDATABLE_HESSIAN) ? pdlp::sessionHessianSlots(*P) : 0;
    f.hasQoff = (opt->updatable & PDLP_UPDATABLE_HESSIAN) ? pdlp::hessianHasOffDiagonalSlot(*P) : pdlp::hessianHasOffDiagonal(*P);
    static const pdlp_update_t kNoData{};
    if (pdlp::residentRoute(opt->updatable, a_value, num_nz, q_value, num_q_nz) == pdlp::kRouteUpdate && !u)
      throw std::runtime_error("pdlp_mi355x_update: null update");
    pdlp::residentUpdateRefusal(f, a_value, num_nz, q_value, num_q_nz, u ? *u : kNoData);
  });
}

// ---- pools (pdlp_pool.hpp) ----------------------------------------------------------------------------------------------
int pdlp_mi355x_solve_many(int32_t K, const pdlp_problem_t* const* P, const pdlp_params_t* opt, int32_t lanes, pdlp_result_t* R,
                           int32_t* path, pdlp_pool_info_t* info) {
  return guarded([&] { pdlp::solveMany(K, P, opt, lanes, R, path, info); });  // (the refusals come before any HIP call)
}

int64_t pdlp_mi355x_pool_info_size(void) { return sizeof(pdlp_pool_info_t); }

// Host twin of the session's decision: what the device finds by streaming the staged arrays against the kept ones is
// found here by walking the two problems; the ladder is the session's own.
int pdlp_mi355x_host_classify(const pdlp_problem_t* held, const pdlp_params_t* held_opt, const pdlp_problem_t* P,
                              const pdlp_params_t* opt, pdlp_session_info_t* out) {
  return guarded([&] {
    if (!P || !opt || !out || (held && !held_opt)) throw std::runtime_error("pdlp_mi355x_host_classify: null argument");
    memset(out, 0, sizeof(*out));
    pdlp::SessionFacts f;
    f.oneShot = pdlp::sessionOneShotReason(*opt);
    f.held = held != nullptr;
    if (!f.oneShot && held) {
      f.changed = pdlp::sessionOptionChanges(*held_opt, *opt);
      if (!(f.changed & PDLP_CHANGED_STRUCTURAL_OPTIONS))
        f.changed |= pdlp::sessionShapeChanges(pdlp::sessionShapeOf(*held), pdlp::sessionShapeOf(*P));
      if (!(f.changed & (PDLP_CHANGED_STRUCTURAL_OPTIONS | PDLP_CHANGED_SHAPE))) {
        pdlp::validateProblem(*held);
        pdlp::validateProblem(*P);
        const pdlp::SessionShape sh = pdlp::sessionShapeOf(*P);
        auto differ = [](const void* a, const void* b, size_t bytes) { return a != b && bytes > 0 && memcmp(a, b, bytes) != 0; };
        const size_t n0 = (size_t)sh.numCol, m = (size_t)sh.numRow, nnz = (size_t)sh.nnz, q = (size_t)sh.qSlots;
        if (differ(held->a_start, P->a_start, 4 * (n0 + 1)) || differ(held->a_index, P->a_index, 4 * nnz)) f.changed |= PDLP_CHANGED_PATTERN;
        if (differ(held->a_value, P->a_value, 8 * nnz)) f.changed |= PDLP_CHANGED_MATRIX_VALUES;
        if (differ(held->col_cost, P->col_cost, 8 * n0)) f.changed |= PDLP_CHANGED_COST;
        if (differ(held->col_lower, P->col_lower, 8 * n0)) f.changed |= PDLP_CHANGED_COL_LOWER;
        if (differ(held->col_upper, P->col_upper, 8 * n0)) f.changed |= PDLP_CHANGED_COL_UPPER;
        if (differ(held->row_lower, P->row_lower, 8 * m) || differ(held->row_upper, P->row_upper, 8 * m)) f.changed |= PDLP_CHANGED_ROW_BOUNDS;
        if (q > 0) {
          if (differ(held->q_start, P->q_start, 4 * ((size_t)sh.qDim + 1)) || differ(held->q_index, P->q_index, 4 * q)) f.changed |= PDLP_CHANGED_HESSIAN_PATTERN;
          if (differ(held->q_value, P->q_value, 8 * q)) f.changed |= PDLP_CHANGED_HESSIAN_VALUES;
        }
        for (int32_t i = 0; i < sh.numRow && f.kindRow < 0; ++i) {
          const int32_t was = pdlp::rowKindOf(held->row_lower[i], held->row_upper[i]), now = pdlp::rowKindOf(P->row_lower[i], P->row_upper[i]);
          if (was != now) { f.kindRow = i; f.kindWas = was; f.kindNow = now; }
        }
      }
    }
    pdlp::sessionLadder(f, out);
  });
}

// MPS ingest (pdlp_mps.cpp).  The arrays of *out are malloc'ed copies owned by the caller's struct.
int pdlp_mi355x_read_mps(const char* path, int32_t num_threads, pdlp_mps_model_t* out) {
  return pdlp_mi355x_read_mps_timed(path, num_threads, 0.0, out);
}

int pdlp_mi355x_read_mps_timed(const char* path, int32_t num_threads, double time_limit, pdlp_mps_model_t* out) {
  int status = 1;
  const int rc = guarded([&] {
    if (!path || !out) throw std::runtime_error("read_mps: NULL argument");
    memset(out, 0, sizeof(*out));
    pdlp::mps::Model M;
    status = pdlp::mps::readMps(path, num_threads, M, time_limit);
    if (status != pdlp::mps::kReadOk) {
      g_lastError = M.error;
      return;
    }
    auto dupStr = [](const std::string& s) {
      char* p = (char*)malloc(s.size() + 1);
      memcpy(p, s.data(), s.size());
      p[s.size()] = 0;
      return p;
    };
    pdlp_problem_t& P = out->lp;
    P.num_col = M.numCol;
    P.num_row = M.numRow;
    P.num_nz = (int64_t)M.aIndex.size();
    P.a_start = dupVec(M.aStart);
    P.a_index = dupVec(M.aIndex);
    P.a_value = dupVec(M.aValue);
    P.col_cost = dupVec(M.colCost);
    P.col_lower = dupVec(M.colLower);
    P.col_upper = dupVec(M.colUpper);
    P.row_lower = dupVec(M.rowLower);
    P.row_upper = dupVec(M.rowUpper);
    P.offset = M.offset;
    P.sense = M.sense;
    if (M.qDim > 0) {
      std::vector<int32_t> qs, qi;
      std::vector<double> qv;
      pdlp::mps::lowerTriangle(M, qs, qi, qv);
      P.q_dim = M.qDim;
      P.q_start = dupVec(qs);
      P.q_index = dupVec(qi);
      P.q_value = dupVec(qv);
      out->hessian_dim = M.qDim;
      out->hessian_start = dupVec(M.qStart);
      out->hessian_index = dupVec(M.qIndex);
      out->hessian_value = dupVec(M.qValue);
    }
    out->cost_row_location = M.costRowLocation;
    if (!M.integrality.empty()) {
      out->num_integrality = M.numCol;
      out->integrality = dupVec(M.integrality);
    }
    out->model_name = dupStr(M.modelName);
    out->objective_name = dupStr(M.objectiveName);
    if (!M.colNameStart.empty()) {
      char* pool = (char*)malloc(M.colNamePool.size() + 1);
      memcpy(pool, M.colNamePool.data(), M.colNamePool.size());
      out->col_name_pool = pool;
      out->col_name_start = dupVec(M.colNameStart);
    }
    if (!M.rowNameStart.empty()) {
      char* pool = (char*)malloc(M.rowNamePool.size() + 1);
      memcpy(pool, M.rowNamePool.data(), M.rowNamePool.size());
      out->row_name_pool = pool;
      out->row_name_start = dupVec(M.rowNameStart);
    }
    out->num_warnings = M.numWarnings;
    out->warning_issued = M.warningIssued ? 1 : 0;
    out->warnings = dupStr(M.warnings);
    out->threads = M.threads;
    out->file_bytes = M.fileBytes;
    out->seconds = M.seconds;
  });
  return rc ? 1 : status;
}

void pdlp_mi355x_free_mps_model(pdlp_mps_model_t* out) {
  if (!out) return;
  pdlp_problem_t& P = out->lp;
  const void* owned[] = {P.a_start, P.a_index, P.a_value, P.col_cost, P.col_lower, P.col_upper, P.row_lower, P.row_upper,
                         P.q_start, P.q_index, P.q_value, out->integrality, out->model_name, out->objective_name,
                         out->col_name_pool, out->col_name_start, out->row_name_pool, out->row_name_start,
                         out->hessian_start, out->hessian_index, out->hessian_value, out->warnings};
  for (const void* p : owned) free((void*)p);
  memset(out, 0, sizeof(*out));
}

int pdlp_mi355x_comm_unique_id(void* id128) {
  return guarded([&] {
    if (!id128) throw std::runtime_error("null argument");
    pdlp::Comm::uniqueId(id128);
  });
}

}  // extern "C"
