// pdlp_session.cpp — pdlp_mi355x_session_* on the host side: the ladder, what a session-held solver keeps and stages
// (Solver::session*), the run-time options of a held solver, and the session itself (see pdlp_session.hpp; the comparison
// kernel is in pdlp_session.hip).
#include "pdlp_session.hpp"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>

#include "pdlp_solver.hpp"
#include "pdlp_update.hpp"

namespace pdlp {

namespace {
const char* shortKind(int32_t k) {
  switch (k) {
    case kRowEq: return "equality";
    case kRowLeq: return "<=";
    case kRowGeq: return ">=";
    case kRowBound: return "ranged or free";
    default: return "unknown";
  }
}

bool sameBits(double a, double b) { return memcmp(&a, &b, sizeof(double)) == 0; }

// "cost, row bounds" from the data bits of a mask
std::string dataNames(int32_t changed) {
  static const struct { int32_t bit; const char* name; } kNames[] = {
      {PDLP_CHANGED_COST, "costs"},           {PDLP_CHANGED_COL_LOWER, "column lower bounds"}, {PDLP_CHANGED_COL_UPPER, "column upper bounds"},
      {PDLP_CHANGED_ROW_BOUNDS, "row bounds"}, {PDLP_CHANGED_OFFSET, "offset"}};
  std::string s;
  for (const auto& e : kNames)
    if (changed & e.bit) s += (s.empty() ? "" : ", ") + std::string(e.name);
  return s;
}
constexpr int32_t kDataBits = PDLP_CHANGED_COST | PDLP_CHANGED_COL_LOWER | PDLP_CHANGED_COL_UPPER | PDLP_CHANGED_ROW_BOUNDS | PDLP_CHANGED_OFFSET;
}  // namespace

void sessionLadder(const SessionFacts& f, pdlp_session_info_t* out) {
  out->path = PDLP_SESSION_NONE;
  out->changed = 0;
  out->kind_row = out->kind_was = out->kind_now = -1;
  out->reserved = 0;
  std::string why;
  if (f.oneShot) {  // rule 1
    out->path = PDLP_SESSION_ONE_SHOT;
    why = std::string("one-shot: ") + f.oneShot;
  } else if (!f.held) {  // rule 2
    out->path = PDLP_SESSION_CREATE;
    why = "create: nothing is held";
  } else {
    out->changed = f.changed;
    const std::string and_ = dataNames(f.changed).empty() ? "" : " (and " + dataNames(f.changed) + ")";
    if (f.changed & PDLP_CHANGED_STRUCTURAL_OPTIONS) {
      out->path = PDLP_SESSION_CREATE;
      why = "create: a structural option differs";
    } else if (f.changed & PDLP_CHANGED_SHAPE) {
      out->path = PDLP_SESSION_CREATE;
      why = "create: sizes, sense or Hessian dimension differ";
    } else if (f.changed & PDLP_CHANGED_PATTERN) {
      out->path = PDLP_SESSION_CREATE;
      why = "create: the matrix pattern differs";
    } else if (f.changed & PDLP_CHANGED_HESSIAN_PATTERN) {
      out->path = PDLP_SESSION_CREATE;
      why = "create: the Hessian pattern differs";
    } else if (f.kindRow >= 0) {
      out->path = PDLP_SESSION_CREATE;
      out->kind_row = f.kindRow; out->kind_was = f.kindWas; out->kind_now = f.kindNow;
      why = "create: row " + std::to_string(f.kindRow) + " changes kind: " + shortKind(f.kindWas) + " -> " + shortKind(f.kindNow);
    } else if (f.changed & PDLP_CHANGED_HESSIAN_VALUES) {  // rule 3
      out->path = PDLP_SESSION_UPDATE_VALUES;
      why = std::string("update values: Hessian values differ") + (f.changed & PDLP_CHANGED_MATRIX_VALUES ? ", matrix values too" : "") + and_;
    } else if (f.changed & PDLP_CHANGED_MATRIX_VALUES) {  // rule 4
      out->path = PDLP_SESSION_UPDATE_MATRIX;
      why = "update matrix: matrix values differ" + and_;
    } else {  // rule 5
      out->path = PDLP_SESSION_UPDATE;
      if (f.changed & kDataBits) why = "update: " + dataNames(f.changed) + " differ" + (f.changed == PDLP_CHANGED_OFFSET ? "s" : "");
      else if (f.changed & PDLP_CHANGED_RUNTIME_OPTIONS) why = "update: only run-time options differ";
      else why = "update: nothing differs";
    }
  }
  snprintf(out->reason, sizeof(out->reason), "%s", why.c_str());
}

const char* sessionOneShotReason(const pdlp_params_t& opt) {
  if (opt.algorithm == 1) return "HiPDLP solvers (algorithm = 1) do not take updates";
  int G = opt.num_devices;
  if (G <= 0) {
    const char* e = getenv("PDLP_MI355X_DEVICES");
    G = e ? atoi(e) : 1;
  }
  if (G > 1) return "sharded solvers (more than one device) do not take updates";
  const char* f = devEnv("PDLP_MI355X_FORCE_COMM");
  if (f && atoi(f) != 0) return "sharded solvers (sharding forced) do not take updates";
  return nullptr;
}

int32_t sessionOptionChanges(const pdlp_params_t& a, const pdlp_params_t& b) {
  int32_t c = 0;
  if (a.device != b.device || a.check_interval != b.check_interval || a.features_off != b.features_off ||
      a.restart_method != b.restart_method || a.algorithm != b.algorithm || a.scaling_mode != b.scaling_mode ||
      a.ruiz_iterations != b.ruiz_iterations || a.step_size_strategy != b.step_size_strategy || a.reserved[0] != b.reserved[0] ||
      a.reserved[1] != b.reserved[1] || a.updatable != b.updatable)
    c |= PDLP_CHANGED_STRUCTURAL_OPTIONS;
  if (!sameBits(a.primal_tol, b.primal_tol) || !sameBits(a.dual_tol, b.dual_tol) || !sameBits(a.gap_tol, b.gap_tol) ||
      !sameBits(a.time_limit, b.time_limit) || a.iter_limit != b.iter_limit || a.log_level != b.log_level ||
      a.log_callback != b.log_callback || a.log_ctx != b.log_ctx)
    c |= PDLP_CHANGED_RUNTIME_OPTIONS;
  return c;
}

int64_t sessionHessianSlots(const pdlp_problem_t& P) {
  return P.q_dim > 0 && P.q_start && P.q_index && P.q_value ? (int64_t)P.q_start[P.q_dim] : 0;
}

SessionShape sessionShapeOf(const pdlp_problem_t& P) {
  SessionShape s;
  s.numCol = P.num_col; s.numRow = P.num_row; s.sense = P.sense; s.qDim = P.q_dim;
  s.nnz = P.num_col > 0 && P.a_start ? (int64_t)P.a_start[P.num_col] : 0;
  s.qSlots = sessionHessianSlots(P);
  s.offset = P.offset;
  return s;
}

int32_t sessionShapeChanges(const SessionShape& a, const SessionShape& b) {
  const bool same = a.numCol == b.numCol && a.numRow == b.numRow && a.nnz == b.nnz && a.sense == b.sense && a.qDim == b.qDim &&
                    a.qSlots == b.qSlots;
  return (same ? 0 : PDLP_CHANGED_SHAPE) | (sameBits(a.offset, b.offset) ? 0 : PDLP_CHANGED_OFFSET);
}

// ---- Solver: run-time options, and what a session keeps and stages ---------------------------------------------------
// The loop reads tolerances and limits from opt_ at the start of every run (uploadCtl, nextCheckIter, checkTermination,
// timeIsUp) and the log sink on every line; nothing that create() captures or plans depends on them: the trial graph
// holds kGraphTrials trials whatever the iteration limit, the check schedule is computed per run.
void Solver::setRuntimeOptions(const pdlp_params_t& opt) {
  opt_.primal_tol = opt.primal_tol;
  opt_.dual_tol = opt.dual_tol;
  opt_.gap_tol = opt.gap_tol;
  opt_.time_limit = opt.time_limit;
  opt_.iter_limit = opt.iter_limit;
  opt_.log_level = opt.log_level;
  opt_.log_callback = opt.log_callback;
  opt_.log_ctx = opt.log_ctx;
}

void Solver::sessionAdopt(const pdlp_problem_t& P) {
  if (!matrixUpdatable_ || mk_.aStart.size() != (size_t)F_.n0 + 1 || mk_.aIndex.size() != (size_t)nnzIn_)
    throw std::runtime_error("pdlp_mi355x_session_solve: the solver kept nothing for matrix updates");
  const int32_t n0 = F_.n0, m = F_.m;
  const int64_t qSlots = sessionHessianSlots(P);
  if (qSlots > 0 && (!hessianUpdatable_ || hk_.nSlots != qSlots))
    throw std::runtime_error("pdlp_mi355x_session_solve: the solver kept nothing for Hessian updates");
  PDLP_HIP(hipSetDevice(opt_.device));
  sessIn_.alloc(DataStage::count(n0, m));
  sessMat_.alloc((size_t)nnzIn_);
  const DataStage d = DataStage::over(sessIn_.get(), n0, m);
  auto put = [&](double* dev, const double* host, int64_t count) {
    if (count > 0) PDLP_HIP(hipMemcpyAsync(dev, host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, stream_));
  };
  put(d.cost, P.col_cost, n0);
  put(d.colLower, P.col_lower, n0);
  put(d.colUpper, P.col_upper, n0);
  put(d.rowLower, P.row_lower, m);
  put(d.rowUpper, P.row_upper, m);
  put(sessMat_.get(), P.a_value, nnzIn_);
  sessQDim_ = 0;
  if (qSlots > 0) {
    sessQDim_ = P.q_dim;
    sessQ_.alloc((size_t)qSlots);
    sessQPat_.alloc((size_t)P.q_dim + 1 + (size_t)qSlots);
    put(sessQ_.get(), P.q_value, qSlots);
    PDLP_HIP(hipMemcpyAsync(sessQPat_.get(), P.q_start, sizeof(int32_t) * ((size_t)P.q_dim + 1), hipMemcpyHostToDevice, stream_));
    PDLP_HIP(hipMemcpyAsync(sessQPat_.get() + P.q_dim + 1, P.q_index, sizeof(int32_t) * (size_t)qSlots, hipMemcpyHostToDevice, stream_));
  }
  sessRec_.alloc(2);
  if (!hostRec_) PDLP_HIP(hipHostMalloc((void**)&hostRec_, 2 * sizeof(int32_t)));
  // the staging buffers every later call fills, with the sizes the updates give them: what is held stays the same from
  // call to call
  ensureDataStaging();
  if (updMat_.size() == 0) updMat_.alloc((size_t)nnzIn_);
  if (qSlots > 0 && updQ_.size() == 0) updQ_.alloc((size_t)qSlots);
  updPat_.alloc((size_t)n0 + 1 + (size_t)nnzIn_ + (qSlots > 0 ? (size_t)P.q_dim + 1 + (size_t)qSlots : 0));
  PDLP_HIP(hipStreamSynchronize(stream_));
}

void Solver::sessionStage(const pdlp_problem_t& P, int32_t* changed, int32_t* kindRow, int32_t* kindWas, double* uploadSeconds) {
  const auto t0 = std::chrono::steady_clock::now();
  if (sessIn_.size() == 0 || !hostRec_) throw std::runtime_error("pdlp_mi355x_session_solve: the solver is not held by a session");
  const int32_t n0 = F_.n0, m = F_.m;
  const int64_t nnz0 = nnzIn_, qSlots = hk_.nSlots > 0 && sessQ_.size() ? hk_.nSlots : 0;
  const size_t nPat = (size_t)n0 + 1 + (size_t)nnz0 + (qSlots > 0 ? (size_t)sessQDim_ + 1 + (size_t)qSlots : 0);
  PDLP_HIP(hipSetDevice(opt_.device));
  PDLP_HIP(hipStreamSynchronize(stream_));
  if (updIn_.size() == 0 || updMat_.size() == 0 || updPat_.size() != nPat || (qSlots > 0 && updQ_.size() == 0))
    throw std::runtime_error("pdlp_mi355x_session_solve: the staging buffers are missing");
  const DataStage in = DataStage::over(updIn_.get(), n0, m), held = DataStage::over(sessIn_.get(), n0, m);
  int32_t* pat = updPat_.get();
  auto put = [&](void* dev, const void* host, size_t bytes) {
    if (bytes > 0) PDLP_HIP(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream_));
  };
  put(pat, P.a_start, sizeof(int32_t) * ((size_t)n0 + 1));
  put(pat + n0 + 1, P.a_index, sizeof(int32_t) * (size_t)nnz0);
  put(in.cost, P.col_cost, sizeof(double) * (size_t)n0);
  put(in.colLower, P.col_lower, sizeof(double) * (size_t)n0);
  put(in.colUpper, P.col_upper, sizeof(double) * (size_t)n0);
  put(in.rowLower, P.row_lower, sizeof(double) * (size_t)m);
  put(in.rowUpper, P.row_upper, sizeof(double) * (size_t)m);
  put(updMat_.get(), P.a_value, sizeof(double) * (size_t)nnz0);
  DiffJobs J;
  auto job = [&](const void* a, const void* b, int64_t count, int32_t width, int32_t bit) {
    if (count <= 0) return;
    DiffJob& j = J.job[J.nJobs++];
    j.a = a; j.b = b; j.count = count; j.width = width; j.bit = bit;
  };
  job(pat, mk_.aStart.get(), (int64_t)n0 + 1, 4, PDLP_CHANGED_PATTERN);
  job(pat + n0 + 1, mk_.aIndex.get(), nnz0, 4, PDLP_CHANGED_PATTERN);
  job(updMat_.get(), sessMat_.get(), nnz0, 8, PDLP_CHANGED_MATRIX_VALUES);
  job(in.cost, held.cost, n0, 8, PDLP_CHANGED_COST);
  job(in.colLower, held.colLower, n0, 8, PDLP_CHANGED_COL_LOWER);
  job(in.colUpper, held.colUpper, n0, 8, PDLP_CHANGED_COL_UPPER);
  job(in.rowLower, held.rowLower, m, 8, PDLP_CHANGED_ROW_BOUNDS);
  job(in.rowUpper, held.rowUpper, m, 8, PDLP_CHANGED_ROW_BOUNDS);
  if (qSlots > 0) {
    int32_t* qpat = pat + n0 + 1 + nnz0;
    put(qpat, P.q_start, sizeof(int32_t) * ((size_t)sessQDim_ + 1));
    put(qpat + sessQDim_ + 1, P.q_index, sizeof(int32_t) * (size_t)qSlots);
    put(updQ_.get(), P.q_value, sizeof(double) * (size_t)qSlots);
    job(qpat, sessQPat_.get(), (int64_t)sessQDim_ + 1 + qSlots, 4, PDLP_CHANGED_HESSIAN_PATTERN);
    job(updQ_.get(), sessQ_.get(), qSlots, 8, PDLP_CHANGED_HESSIAN_VALUES);
  }
  PDLP_HIP(hipStreamSynchronize(stream_));  // (only to tell the uploads' time from the comparison's)
  *uploadSeconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  J.rowLower = in.rowLower;
  J.rowUpper = in.rowUpper;
  J.rowKind = rowKindDev_.get();
  J.m = m;
  hostRec_[0] = 0;
  hostRec_[1] = m;
  PDLP_HIP(hipMemcpyAsync(sessRec_.get(), hostRec_, 2 * sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  launchSessionDiff(J, sessRec_.get(), stream_);
  PDLP_HIP(hipMemcpyAsync(hostRec_, sessRec_.get(), 2 * sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
  PDLP_HIP(hipStreamSynchronize(stream_));
  *changed = hostRec_[0];
  const int32_t bad = hostRec_[1];
  *kindRow = bad >= 0 && bad < m ? bad : -1;
  *kindWas = *kindRow >= 0 ? F_.rowKind[(size_t)bad] : -1;
}

void Solver::sessionCommit() {
  std::swap(updIn_, sessIn_);
  std::swap(updMat_, sessMat_);
  if (sessQ_.size()) std::swap(updQ_, sessQ_);
}

size_t Solver::sessionHeldBytes() const {
  return dataKeptBytes() + matrixKeptBytes() + hessianKeptBytes() +  // ... and the session's own six buffers
         sizeof(double) * (sessIn_.size() + sessMat_.size() + sessQ_.size()) +
         sizeof(int32_t) * (sessQPat_.size() + updPat_.size() + sessRec_.size());
}

// ---- the session ------------------------------------------------------------------------------------------------------
Session::Session() {
  info_.path = PDLP_SESSION_NONE;
  info_.kind_row = info_.kind_was = info_.kind_now = -1;
  snprintf(info_.reason, sizeof(info_.reason), "nothing solved yet");
}
Session::~Session() { release(); }

void Session::release() noexcept {
  try {
    delete solver_;
  } catch (...) {
  }
  solver_ = nullptr;
}

// The create path: whatever is held is destroyed first; the new solver keeps what every update needs and the caller's arrays.
void Session::create(const pdlp_problem_t& P, const pdlp_params_t& opt) {
  release();
  pdlp_params_t o = opt;
  o.updatable |= PDLP_UPDATABLE_DATA | PDLP_UPDATABLE_MATRIX;
  if (sessionHessianSlots(P) > 0) o.updatable |= PDLP_UPDATABLE_HESSIAN;
  Solver* s = new Solver(P, o, 0, 1, nullptr);
  try {
    s->sessionAdopt(P);
  } catch (...) {
    delete s;
    throw;
  }
  solver_ = s;
}

// Rules 2-5 against the held solver: the options and the shape on the host, the arrays on the device (only when options
// and shape allow reuse at all: the staging buffers have the held problem's sizes).
void Session::findChanges(const pdlp_problem_t& P, const pdlp_params_t& opt, SessionFacts& f) {
  f.changed = sessionOptionChanges(heldOpt_, opt);
  if (f.changed & PDLP_CHANGED_STRUCTURAL_OPTIONS) return;
  f.changed |= sessionShapeChanges(held_, sessionShapeOf(P));
  if (f.changed & PDLP_CHANGED_SHAPE) return;
  // (the shape is the held one: what create's validateProblem asks of the pointers; equal patterns need no second look)
  if (P.num_col > 0 && (!P.a_start || !P.col_cost || !P.col_lower || !P.col_upper)) throw std::runtime_error("null column arrays");
  if (P.num_row > 0 && (!P.row_lower || !P.row_upper)) throw std::runtime_error("null row arrays");
  if (held_.nnz > 0 && (!P.a_index || !P.a_value)) throw std::runtime_error("null matrix arrays");
  using clock = std::chrono::steady_clock;
  const auto t1 = clock::now();
  int32_t arrays = 0;
  solver_->sessionStage(P, &arrays, &f.kindRow, &f.kindWas, &info_.upload_seconds);
  f.changed |= arrays;
  if (f.kindRow >= 0) f.kindNow = rowKindOf(P.row_lower[f.kindRow], P.row_upper[f.kindRow]);
  info_.diff_seconds = std::chrono::duration<double>(clock::now() - t1).count();
}

// The chosen update, from the staged arrays, with exactly the arrays that differ.
void Session::applyReuse(const pdlp_problem_t& P, const pdlp_params_t& opt, int32_t c) {
  pdlp_update_t u{};
  if (c & PDLP_CHANGED_COST) u.col_cost = P.col_cost;
  if (c & PDLP_CHANGED_COL_LOWER) u.col_lower = P.col_lower;
  if (c & PDLP_CHANGED_COL_UPPER) u.col_upper = P.col_upper;
  if (c & PDLP_CHANGED_ROW_BOUNDS) { u.row_lower = P.row_lower; u.row_upper = P.row_upper; }
  if (c & PDLP_CHANGED_OFFSET) { u.offset = P.offset; u.has_offset = 1; }
  if (P.start_value_valid && P.start_dual_valid && P.start_col_value && P.start_row_value && P.start_row_dual) {
    u.start_col_value = P.start_col_value; u.start_row_value = P.start_row_value; u.start_row_dual = P.start_row_dual;
  }
  const double* aValue = c & PDLP_CHANGED_MATRIX_VALUES ? P.a_value : nullptr;
  const int64_t numNz = aValue ? held_.nnz : 0;
  solver_->setRuntimeOptions(opt);
  solver_->sessionSetStaged(true);
  if (info_.path == PDLP_SESSION_UPDATE_VALUES) solver_->updateValues(aValue, numNz, P.q_value, held_.qSlots, &u);
  else if (info_.path == PDLP_SESSION_UPDATE_MATRIX) solver_->updateMatrix(aValue, numNz, &u);
  else solver_->update(u);
  solver_->sessionSetStaged(false);
  solver_->sessionCommit();
}

int Session::solve(const pdlp_problem_t& P, const pdlp_params_t& opt, pdlp_result_t* R) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  auto since = [](clock::time_point a) { return std::chrono::duration<double>(clock::now() - a).count(); };
  auto say = [&] { if (opt.log_level >= 1) logLine(opt, 1, "Session: %s\n", info_.reason); };
  SessionFacts f;
  f.oneShot = sessionOneShotReason(opt);
  info_.diff_seconds = info_.upload_seconds = info_.apply_seconds = info_.setup_seconds = 0.0;
  info_.held_bytes = 0;
  if (f.oneShot) {
    release();
    sessionLadder(f, &info_);
    say();
    const int rc = pdlp_mi355x_solve(&P, &opt, R);
    if (rc == 0 && R) info_.setup_seconds = R->setup_seconds;
    return rc;
  }
  try {
    f.held = solver_ != nullptr;
    std::string failure;
    bool failed = false;
    auto t1 = clock::now();
    try {
      if (f.held) findChanges(P, opt, f);
      sessionLadder(f, &info_);
      say();
      t1 = clock::now();
      if (info_.path != PDLP_SESSION_CREATE) applyReuse(P, opt, f.changed);
    } catch (const std::exception& e) {  // a reuse path failed, for whatever reason: the create path, once
      failed = true;
      failure = e.what();
    }
    if (failed) {
      std::string why = "create: the reuse path failed (" + failure;
      if (why.size() > sizeof(info_.reason) - 2) why.resize(sizeof(info_.reason) - 2);
      why += ")";
      info_.path = PDLP_SESSION_CREATE;
      snprintf(info_.reason, sizeof(info_.reason), "%s", why.c_str());
      say();
    }
    if (info_.path == PDLP_SESSION_CREATE) create(P, opt);
    info_.apply_seconds = since(t1);
    heldOpt_ = opt;
    held_ = sessionShapeOf(P);
    info_.held_bytes = (int64_t)solver_->sessionHeldBytes();
    info_.setup_seconds = since(t0);
    solver_->run(R);
    if (R) R->setup_seconds = info_.setup_seconds;
  } catch (...) {  // after a failure the session holds nothing
    release();
    info_.held_bytes = 0;
    throw;
  }
  return 0;
}

}  // namespace pdlp
