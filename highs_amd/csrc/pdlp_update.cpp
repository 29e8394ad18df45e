// pdlp_update.cpp — pdlp_mi355x_update on the host side: validation, the host restatement of the replay, and
// Solver::update (see pdlp_update.hpp; the kernels are in pdlp_update.hip).
#include "pdlp_update.hpp"

#include <chrono>
#include <cstring>
#include <limits>
#include <stdexcept>
#include <string>

#include "pdlp_solver.hpp"

namespace pdlp {

namespace {
const char* kindName(int32_t k) {
  switch (k) {
    case kRowEq: return "equality";
    case kRowLeq: return "<= (upper bound only)";
    case kRowGeq: return ">= (lower bound only)";
    case kRowBound: return "ranged or free";
    default: return "unknown";
  }
}
[[noreturn]] void refuse(const char* entry, const char* sentence) { throw std::runtime_error(std::string(entry) + ": " + sentence); }
}  // namespace

void refuseHipdlp(const char* entry) { refuse(entry, "HiPDLP solvers (algorithm = 1) do not take updates"); }
void refuseSharded(const char* entry) { refuse(entry, "sharded solvers (pdlp_mi355x_create_sharded) do not take updates"); }
void refuseNotUpdatable(const char* entry) { refuse(entry, "the solver was not created for updates (pdlp_params_t.updatable = 0)"); }
void refuseNoMatrixBit(const char* entry) {
  const std::string given = entry == std::string(kEntryUpdateValues) ? "a_value given, but " : "";
  refuse(entry, (given + "the solver was not created for matrix updates (pdlp_params_t.updatable lacks PDLP_UPDATABLE_MATRIX)").c_str());
}
void refuseNoHessianBit(const char* entry) {
  refuse(entry, "the solver was not created for Hessian updates (pdlp_params_t.updatable lacks PDLP_UPDATABLE_HESSIAN)");
}
void refuseOffDiagonalHessian(const char* entry) {
  refuse(entry, "QPs whose Hessian has off-diagonal entries do not take matrix updates (the scaled copy of the Hessian follows "
                "the column factors; left for a later change)");
}

void checkUpdateShape(const pdlp_update_t& u) {
  if ((u.row_lower != nullptr) != (u.row_upper != nullptr))
    throw std::runtime_error(std::string("pdlp_mi355x_update: row_lower and row_upper are given together or not at all (") +
                             (u.row_lower ? "row_upper" : "row_lower") + " is NULL)");
  const int given = (u.start_col_value ? 1 : 0) + (u.start_row_value ? 1 : 0) + (u.start_row_dual ? 1 : 0);
  if (given != 0 && given != 3)
    throw std::runtime_error("pdlp_mi355x_update: partial start: start_col_value, start_row_value and start_row_dual are given "
                             "all three (hot start) or none (cold start), " + std::to_string(given) + " of 3 are given");
}

void refuseKindChange(const int32_t* rowKind, int32_t m, const double* rowLower, const double* rowUpper) {
  for (int32_t i = 0; i < m; ++i)
    if (rowKindOf(rowLower[i], rowUpper[i]) != rowKind[i]) refuseKindChangeAt(rowKind, i, rowLower, rowUpper);
}

void refuseKindChangeAt(const int32_t* rowKind, int32_t row, const double* rowLower, const double* rowUpper) {
  refuseKindChangeAt(rowKind[row], row, rowLower[row], rowUpper[row]);
}

void refuseKindChangeAt(int32_t kindWas, int32_t row, double lower, double upper) {
  throw std::runtime_error("pdlp_mi355x_update: row " + std::to_string(row) + " would change its kind from " + kindName(kindWas) +
                           " to " + kindName(rowKindOf(lower, upper)) +
                           " (the kind decides row order, slack columns and signs: create a new solver)");
}

void hostReplayUpdate(const pdlp_update_t& u, StandardForm& F) {
  checkUpdateShape(u);
  if (!F.keepPasses) throw std::runtime_error("pdlp_mi355x_update: the form did not keep its scaling passes");
  const int32_t n0 = F.n0, n = F.n, m = F.m;
  const int32_t mask = updateMask(u);
  if (mask & kUpdRows) refuseKindChange(F.rowKind.data(), m, u.row_lower, u.row_upper);
  const double kInf = std::numeric_limits<double>::infinity();
  auto infLo = [&](double v) { return v < -1e20 ? -kInf : v; };
  auto infUp = [&](double v) { return v > 1e20 ? kInf : v; };
  // the columns, as k_update_cols takes them
  std::vector<int32_t> slackRow;
  for (int32_t i = 0; i < m; ++i)
    if (F.rowKind[i] == kRowBound) slackRow.push_back(i);
  for (int32_t j = 0; j < n; ++j) {
    bool dc = false, dl = false, du = false;
    double c = 0.0, lo = 0.0, up = 0.0;
    if (j < n0) {
      dc = mask & kUpdCost; dl = mask & kUpdColLower; du = mask & kUpdColUpper;
      if (dc) c = u.col_cost[j] * F.sense;
      if (dl) lo = infLo(u.col_lower[j]);
      if (du) up = infUp(u.col_upper[j]);
    } else if (mask & kUpdRows) {
      dl = du = true;
      const int32_t r = slackRow[(size_t)(j - n0)];
      lo = infLo(u.row_lower[r]);
      up = infUp(u.row_upper[r]);
    }
    if (!F.cost0.empty()) {  // matrix-updatable form: the unscaled data follow every update
      if (dc) F.cost0[j] = c;
      if (dl) F.lower0[j] = lo;
      if (du) F.upper0[j] = up;
    }
    for (int32_t p = 0; p < F.nPass; ++p) {
      const double cs = F.csPass[(size_t)p * n + j];
      c /= cs; lo *= cs; up *= cs;
    }
    if (dc) F.cost[j] = c;
    if (dl) F.lower[j] = lo;
    if (du) F.upper[j] = up;
  }
  if (mask & kUpdRows)
    for (int32_t i = 0; i < m; ++i) {
      const int32_t ni = F.rowNewIdx[i], k = F.rowKind[i];
      double r;
      if (k == kRowEq) r = u.row_lower[i];
      else if (k == kRowBound) r = 0.0;
      else if (k == kRowLeq) r = -u.row_upper[i];
      else r = u.row_lower[i];
      if (!F.rhs0.empty()) F.rhs0[ni] = r;
      for (int32_t p = 0; p < F.nPass; ++p) r /= F.rsPass[(size_t)p * m + ni];
      F.rhs[ni] = r;
    }
  if (mask & kUpdCost) F.normCost = unscaledNormCost(u.col_cost, n0, F.sense);
  if (mask & kUpdRows) F.normRhs = unscaledNormRhs(u.row_lower, u.row_upper, F.rowKind.data(), m);
  if (u.has_offset) F.offset = u.offset;
}

void keepUnscaled(StandardForm& F) {
  F.cost0 = F.cost; F.lower0 = F.lower; F.upper0 = F.upper; F.rhs0 = F.rhs; F.qdiag0 = F.qdiag;
}

void throwAllZeroMatrix() {  // the wording of requireConstraints (pdlp_host.cpp): what create() says to such a matrix
  throw std::runtime_error("pdlp_mi355x: the LP has no rows, no columns or no matrix nonzeros — HiGHS solves such "
                           "LPs itself (solveUnconstrainedLp) before the PDLP path");
}

void checkMatrixUpdateShape(const double* aValue, int64_t numNz, int64_t nnzAtCreate) {
  if (!aValue) throw std::runtime_error("pdlp_mi355x_update_matrix: a_value is NULL");
  if (numNz != nnzAtCreate)
    throw std::runtime_error("pdlp_mi355x_update_matrix: num_nz = " + std::to_string(numNz) + " differs from the " +
                             std::to_string(nnzAtCreate) + " nonzeros the solver was created with (the sparsity pattern is fixed: "
                             "create a new solver)");
}

void keepUnscaledHessian(StandardForm& F) {
  F.qdiag0 = F.qdiag;
  F.qoff0 = F.qoff.val;
}

void checkHessianUpdateShape(const double* qValue, int64_t numQNz, bool hasHessian, int64_t slotsAtCreate) {
  if (!qValue) {
    if (numQNz != 0)
      throw std::runtime_error("pdlp_mi355x_update_values: q_value is NULL but num_q_nz = " + std::to_string(numQNz));
    return;
  }
  if (!hasHessian)
    throw std::runtime_error("pdlp_mi355x_update_values: q_value given to a solver that was created without a Hessian (the "
                             "sparsity pattern is fixed: create a new solver)");
  if (numQNz != slotsAtCreate)
    throw std::runtime_error("pdlp_mi355x_update_values: num_q_nz = " + std::to_string(numQNz) + " differs from the " +
                             std::to_string(slotsAtCreate) + " Hessian slots the solver was created with (the sparsity pattern is "
                             "fixed: create a new solver)");
}

void throwNegativeDiagonal(int32_t col) {
  throw std::runtime_error("pdlp_mi355x_update_values: the Hessian is not positive semidefinite for this objective sense (the "
                           "diagonal entry of column " + std::to_string(col) + " is negative)");
}

// Solver::updateValues' refusals, then those of the Impl it hands over to (updateMatrixImpl with a_value, else updateImpl),
// up to the point where either looks at a value
void refuseValueUpdate(const ValueUpdateFacts& f, const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz,
                       const pdlp_update_t& u) {
  const bool matrixBit = (f.updatable & PDLP_UPDATABLE_MATRIX) != 0, hessianBit = (f.updatable & PDLP_UPDATABLE_HESSIAN) != 0;
  const bool asMatrix = aValue && !qValue && numQNz == 0 && !hessianBit;  // pdlp_mi355x_update_matrix (Solver::updateMatrix)
  if (!asMatrix) {
    if (f.sharded) refuseSharded(kEntryUpdateValues);
    if (!hessianBit) refuseNoHessianBit(kEntryUpdateValues);
    if (!aValue && numNz != 0)
      throw std::runtime_error("pdlp_mi355x_update_values: a_value is NULL but num_nz = " + std::to_string(numNz));
    if (aValue && !matrixBit) refuseNoMatrixBit(kEntryUpdateValues);
    checkHessianUpdateShape(qValue, numQNz, f.qSlots > 0, f.qSlots);
  }
  if (aValue) {
    if (f.sharded) refuseSharded(kEntryUpdateMatrix);
    if (!matrixBit) refuseNoMatrixBit(kEntryUpdateMatrix);
    if (f.hasQoff && !hessianBit) refuseOffDiagonalHessian(kEntryUpdateMatrix);
    checkMatrixUpdateShape(aValue, numNz, f.nnz);
  } else if (!f.updatable) {
    refuseNotUpdatable(kEntryUpdate);
  }
  checkUpdateShape(u);
  if (u.row_lower) refuseKindChange(f.rowKind, f.m, u.row_lower, u.row_upper);
}

void hostAssembleHessianUpdate(const double* qValue, StandardForm& F, bool validateOnly) {
  if (!F.hmap.kept() || F.qdiag0.size() != (size_t)F.n || F.qoff0.size() != (size_t)F.hmap.nOff)
    throw std::runtime_error("pdlp_mi355x_update_values: the form did not keep its Hessian");
  const int32_t bad = firstNegativeDiagonal(F.hmap, qValue, F.sense);
  if (bad < F.n) throwNegativeDiagonal(bad);
  if (validateOnly) return;
  assembleHessian(F.hmap, qValue, F.sense, F.qdiag0.data(), F.qoff0.data());
}

void hostReplayHessianUpdate(const double* qValue, StandardForm& F) {
  if (!F.keepPasses) throw std::runtime_error("pdlp_mi355x_update_values: the form did not keep its scaling passes");
  hostAssembleHessianUpdate(qValue, F, false);
  const int32_t n = F.n;
  for (int32_t j = 0; j < n; ++j) {  // as k_hessian_replay takes them
    double d = F.qdiag0[j];
    for (int32_t p = 0; p < F.nPass; ++p) { const double cs = F.csPass[(size_t)p * n + j]; d = (d / cs) / cs; }
    F.qdiag[j] = d;
  }
  for (int32_t k = 0; k < F.hmap.nOff; ++k) {
    const int32_t r = F.hmap.offRow[k], c = F.hmap.offCol[k];
    double v = F.qoff0[k];
    for (int32_t p = 0; p < F.nPass; ++p) v = (v / F.csPass[(size_t)p * n + r]) / F.csPass[(size_t)p * n + c];
    F.qoff.val[k] = v;
  }
}

void hostReplayMatrixUpdate(const pdlp_problem_t& P, const double* aValue, const pdlp_update_t* u, bool doScale, StandardForm& F,
                            const double* qValue) {
  const int64_t nnz0 = F.n0 > 0 ? (int64_t)P.a_start[F.n0] : 0;
  if (!aValue) throw std::runtime_error("pdlp_mi355x_update_matrix: a_value is NULL");
  if (!F.keepPasses || F.cost0.size() != F.cost.size())
    throw std::runtime_error("pdlp_mi355x_update_matrix: the form did not keep its unscaled data");
  if (u) {
    checkUpdateShape(*u);
    if (updateMask(*u) & kUpdRows) refuseKindChange(F.rowKind.data(), F.m, u->row_lower, u->row_upper);
  }
  bool anyNonzero = false;
  for (int64_t p = 0; p < nnz0 && !anyNonzero; ++p) anyNonzero = aValue[p] != 0.0;
  if (!anyNonzero) throwAllZeroMatrix();
  if (qValue) hostAssembleHessianUpdate(qValue, F, true);
  // ---- nothing below is refused ----
  formulateValues(P.a_start, P.a_index, aValue, F);
  if (qValue) hostAssembleHessianUpdate(qValue, F, false);
  F.cost = F.cost0; F.lower = F.lower0; F.upper = F.upper0; F.rhs = F.rhs0; F.qdiag = F.qdiag0;
  if (F.hmap.kept() && F.hmap.nOff > 0) F.qoff.val = F.qoff0;  // (a Hessian-updatable form: scale() below takes the off-diagonal part along)
  F.colScale.assign((size_t)F.n, 1.0);
  F.rowScale.assign((size_t)F.m, 1.0);
  F.nPass = 0;
  F.csPass.clear();
  F.rsPass.clear();
  F.scaled = false;
  if (u) hostReplayUpdate(*u, F);  // (no pass is kept at this point: the formulated data, unscaled, and their norms)
  if (doScale) scale(F);           // the set-up's own passes; keeps the NEW factors for later updates
}

void SolverBase::update(const pdlp_update_t&) { refuseHipdlp(kEntryUpdate); }
void SolverBase::updateMatrix(const double*, int64_t, const pdlp_update_t*) { refuseHipdlp(kEntryUpdateMatrix); }
void SolverBase::updateValues(const double*, int64_t, const double*, int64_t, const pdlp_update_t*) { refuseHipdlp(kEntryUpdateValues); }

void SolverBase::setRuntimeOptions(const pdlp_params_t&) {
  throw std::runtime_error("pdlp_mi355x: HiPDLP solvers (algorithm = 1) are not held across solves: no new options");
}

namespace {
using clock = std::chrono::steady_clock;
double since(clock::time_point a) { return std::chrono::duration<double>(clock::now() - a).count(); }
}  // namespace

// ---- what the update entries share: the staging head, the scaled sums, the finishing tail --------------------------------
size_t Solver::dataKeptBytes() const {
  return sizeof(double) * (csPass_.size() + rsPass_.size() + updIn_.size()) +
         sizeof(int32_t) * (rowKindDev_.size() + rowNewIdxDev_.size() + slackRowDev_.size() + updBad_.size());
}
size_t Solver::matrixKeptBytes() const {
  return mk_.bytes() + sizeof(int32_t) * (srcAVal_.size() + srcASlab_.size() + srcAtVal_.size() + srcAtSlab_.size()) +
         sizeof(double) * updMat_.size();
}
size_t Solver::hessianKeptBytes() const {
  return hk_.bytes() + sizeof(int32_t) * (srcQVal_.size() + srcQSlab_.size()) + sizeof(double) * updQ_.size();
}

void Solver::ensureDataStaging() {
  if (updIn_.size() != 0) return;
  updIn_.alloc(DataStage::count(F_.n0, F_.m));
  updBad_.alloc(1);
}

void Solver::stagePut(double* dev, const double* host, int64_t count) {  // (a session has staged them already)
  if (count > 0 && !staged_) PDLP_HIP(hipMemcpyAsync(dev, host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, stream_));
}

// The head: the caller's row bounds into the staging buffer, the validation kernel on that and the kept kinds.  Nothing
// of the solver is written.
void Solver::stageRowsAndValidate(const pdlp_update_t& ud, int32_t mask, const DataStage& D) {
  if (!(mask & kUpdRows)) return;
  const int32_t m = F_.m;
  stagePut(D.rowLower, ud.row_lower, m);
  stagePut(D.rowUpper, ud.row_upper, m);
  int32_t bad = m;
  PDLP_HIP(hipMemcpyAsync(updBad_.get(), &bad, sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  launchUpdateValidate(D.rowLower, D.rowUpper, rowKindDev_.get(), m, updBad_.get(), stream_);
  PDLP_HIP(hipMemcpyAsync(&bad, updBad_.get(), sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
  PDLP_HIP(hipStreamSynchronize(stream_));
  if (bad < m) refuseKindChangeAt(F_.rowKind.data(), bad, ud.row_lower, ud.row_upper);
}

void Solver::stageColumns(const pdlp_update_t& ud, int32_t mask, const DataStage& D) {
  if (mask & kUpdCost) stagePut(D.cost, ud.col_cost, F_.n0);
  if (mask & kUpdColLower) stagePut(D.colLower, ud.col_lower, F_.n0);
  if (mask & kUpdColUpper) stagePut(D.colUpper, ud.col_upper, F_.n0);
}

// The staged data into cost / lower / upper / rhs through the nPass passes (nullptr, 0: the unscaled copies)
void Solver::replayData(int32_t mask, const DataStage& D, const double* csPass, const double* rsPass, int32_t nPass, double* cost,
                        double* lower, double* upper, double* rhs) {
  launchUpdateCols(mask, D.cost, D.colLower, D.colUpper, D.rowLower, D.rowUpper, slackRowDev_.get(), F_.sense, F_.n0, F_.n, csPass,
                   nPass, cost, lower, upper, stream_);
  if (mask & kUpdRows)
    launchUpdateRows(D.rowLower, D.rowUpper, rowKindDev_.get(), rowNewIdxDev_.get(), F_.m, rsPass, nPass, rhs, stream_);
}

// The left-to-right sums of the scaled c, b (PDHG_Init_Step_Sizes), by the host loops of the set-up
void Solver::refreshScaledSums(bool cost, bool rhs) {
  std::vector<double> hc(cost ? (size_t)F_.n : 0), hb(rhs ? (size_t)F_.m : 0);
  cost_.download(hc.data(), hc.size(), stream_);
  rhs_.download(hb.data(), hb.size(), stream_);
  PDLP_HIP(hipStreamSynchronize(stream_));
  if (cost) sumCost2_ = 0.0;
  for (double v : hc) sumCost2_ += v * v;
  if (rhs) sumRhs2_ = 0.0;
  for (double v : hb) sumRhs2_ += v * v;
}

// The fused slab trial's per-block bounds; the captured batch bakes IterVecs::lowerUniform in (the vectors' addresses have
// not changed), so only a flip of that flag needs a new graph
bool Solver::refreshBoundsFlipsUniform() {
  const int32_t before = vecs_.lowerUniform;
  const int32_t after = refreshBlockBounds() ? 1 : 0;
  return before != after;
}

// The tail: the start of the next run, reset, a new graph where `recapture` asks for one
void Solver::finishUpdate(const pdlp_update_t& ud, bool recapture, double* resetSeconds, double* captureSeconds,
                          std::chrono::steady_clock::time_point t0) {
  if (ud.start_col_value) {
    setHotStart(ud.start_col_value, ud.start_row_value, ud.start_row_dual);  // (with the scale vectors as they are now)
  } else {
    hasStart_ = false;
    startX_.clear();
    startY_.clear();
  }
  auto t1 = clock::now();
  stPar_ = graphExec_ && !recapture ? graphPar_ : 0;  // the state slot a fresh solver starts from / the kept graph was captured with
  reset();
  stalledRounds_ = 0;
  stalledSince_ = 0;
  *resetSeconds = since(t1);
  t1 = clock::now();
  if (recapture && graphExec_) {
    (void)hipGraphExecDestroy(graphExec_);
    graphExec_ = nullptr;
    captureGraph();
  }
  PDLP_HIP(hipStreamSynchronize(stream_));
  *captureSeconds = since(t1);
  updRecaptured_ = recapture && graphExec_ ? 1 : 0;
  setupSeconds_ = since(t0);
}

// The held solver is brought to the state of a fresh create() on the modified problem.  Everything that can be refused
// is refused before the first write to the solver's vectors.
void Solver::update(const pdlp_update_t& u) { updateImpl(u, nullptr); }

// qValue (or nullptr): new Hessian values as well (pdlp_mi355x_update_values without a_value; the count is checked there)
void Solver::updateImpl(const pdlp_update_t& u, const double* qValue) {
  const auto t0 = clock::now();
  if (sharded_) refuseSharded(kEntryUpdate);
  if (!updatable_) refuseNotUpdatable(kEntryUpdate);
  checkUpdateShape(u);
  const int32_t mask = updateMask(u);
  PDLP_HIP(hipSetDevice(opt_.device));
  PDLP_HIP(hipStreamSynchronize(stream_));
  ensureDataStaging();
  const DataStage D = DataStage::over(updIn_.get(), F_.n0, F_.m);
  stageRowsAndValidate(u, mask, D);
  if (qValue) stageHessian(qValue);
  // ---- nothing below is refused ----
  stageColumns(u, mask, D);
  PDLP_HIP(hipStreamSynchronize(stream_));
  updSeconds_[kUpdStage] = since(t0);

  auto t1 = clock::now();
  replayData(mask, D, csPass_.get(), rsPass_.get(), nPass_, cost_.get(), lower_.get(), upper_.get(), rhs_.get());
  if (matrixUpdatable_)  // the unscaled data follow every update: the same kernels with no pass to replay
    replayData(mask, D, nullptr, nullptr, 0, mk_.cost0.get(), mk_.lower0.get(), mk_.upper0.get(), mk_.rhs0.get());
  PDLP_HIP(hipStreamSynchronize(stream_));
  updSeconds_[kUpdKernels] = since(t1);
  // the Hessian: assembled from the staging copy, taken through the kept passes (the matrix, so every factor, stays)
  if (qValue) applyHessian(true, true);

  // termination norms of the unscaled data and the sums of the scaled c, b
  t1 = clock::now();
  if (mask & kUpdCost) {
    F_.normCost = unscaledNormCost(u.col_cost, F_.n0, F_.sense);
    refreshScaledSums(true, false);
  }
  if (mask & kUpdRows) {
    F_.normRhs = unscaledNormRhs(u.row_lower, u.row_upper, F_.rowKind.data(), F_.m);
    refreshScaledSums(false, true);
  }
  if (u.has_offset) F_.offset = u.offset;
  updSeconds_[kUpdSums] = since(t1);

  t1 = clock::now();
  const bool recapture = fused_ && (mask & (kUpdColLower | kUpdColUpper | kUpdRows)) && refreshBoundsFlipsUniform();
  updSeconds_[kUpdBounds] = since(t1);
  finishUpdate(u, recapture, &updSeconds_[kUpdReset], &updSeconds_[kUpdCapture], t0);
}

// pdlp_mi355x_update_values: a_value, q_value and u, each optional, as ONE change.  The refusals that depend on how the
// solver was created come first; the rest is the data update or the matrix update with the Hessian's part in it.
void Solver::updateValues(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u) {
  if (sharded_) refuseSharded(kEntryUpdateValues);
  if (!(opt_.updatable & PDLP_UPDATABLE_HESSIAN)) refuseNoHessianBit(kEntryUpdateValues);
  if (!aValue && numNz != 0)
    throw std::runtime_error("pdlp_mi355x_update_values: a_value is NULL but num_nz = " + std::to_string(numNz));
  if (aValue && !(opt_.updatable & PDLP_UPDATABLE_MATRIX)) refuseNoMatrixBit(kEntryUpdateValues);
  checkHessianUpdateShape(qValue, numQNz, hk_.nSlots > 0, hk_.nSlots);
  for (double& s : updHessSeconds_) s = 0.0;
  if (aValue) {
    updateMatrixImpl(aValue, numNz, u, qValue);
  } else {
    static const pdlp_update_t kNoData{};
    updateImpl(u ? *u : kNoData, qValue);
  }
}

// The caller's q_value into its staging buffer and the validation kernel on it: nothing of the solver is written.
void Solver::stageHessian(const double* qValue) {
  const auto t0 = clock::now();
  const int32_t n = F_.n;
  if (updQ_.size() == 0) updQ_.alloc((size_t)hk_.nSlots);
  stagePut(updQ_.get(), qValue, hk_.nSlots);
  int32_t bad = n;  // (updBad_: ensureDataStaging, which every caller has been through)
  PDLP_HIP(hipMemcpyAsync(updBad_.get(), &bad, sizeof(int32_t), hipMemcpyHostToDevice, stream_));
  launchHessianValidate(hk_.dstBeg.get(), hk_.srcSlot.get(), updQ_.get(), F_.sense, n, updBad_.get(), stream_);
  PDLP_HIP(hipMemcpyAsync(&bad, updBad_.get(), sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
  PDLP_HIP(hipStreamSynchronize(stream_));
  updHessSeconds_[kHessStage] = since(t0);
  if (bad < n) throwNegativeDiagonal(bad);
}

// assemble: qdiag0 / qoff0 from the staged q_value.  replayDiag: qdiag_ from qdiag0 through the kept passes (a matrix
// update leaves the diagonal to its scaling passes instead).  Always: the off-diagonal part through csPass_ as it stands,
// and dQ_'s value arrays refilled from it.
void Solver::applyHessian(bool assemble, bool replayDiag) {
  const int32_t n = F_.n, nOff = hk_.nOff;
  double* qdiag0 = qdiag0Dev();
  auto t1 = clock::now();
  if (assemble) {
    launchHessianAssemble(hk_.dstBeg.get(), hk_.srcSlot.get(), updQ_.get(), F_.sense, n, nOff, qdiag0, hk_.qoff0.get(), stream_);
    PDLP_HIP(hipStreamSynchronize(stream_));
    updHessSeconds_[kHessAssemble] = since(t1);
  }
  t1 = clock::now();
  const double* diagSrc = replayDiag ? qdiag0 : nullptr;
  const double* offSrc = nOff > 0 ? hk_.qoff0.get() : nullptr;
  if (F_.scaled) {
    launchHessianReplay(diagSrc, offSrc, hk_.offRow.get(), hk_.offCol.get(), n, nOff, csPass_.get(), nPass_, qdiag_.get(),
                        hk_.qoffScaled.get(), stream_);
  } else {  // (PDLP_FEATURE_SCALING_OFF: nothing is replayed)
    if (diagSrc) PDLP_HIP(hipMemcpyAsync(qdiag_.get(), diagSrc, sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, stream_));
    if (offSrc) PDLP_HIP(hipMemcpyAsync(hk_.qoffScaled.get(), offSrc, sizeof(double) * (size_t)nOff, hipMemcpyDeviceToDevice, stream_));
  }
  PDLP_HIP(hipStreamSynchronize(stream_));
  updHessSeconds_[kHessReplay] = since(t1);
  t1 = clock::now();
  if (nOff > 0) refillHessian();
  PDLP_HIP(hipStreamSynchronize(stream_));
  updHessSeconds_[kHessRefill] = since(t1);
}

// pdlp_mi355x_update_matrix: new matrix values on the kept pattern, optionally with new data (u), as ONE change.  Of
// create()'s work only the value-dependent layer runs: formulate values -> the set-up's pass loop -> matNormInf -> one
// refill per value array.  No sort, no layout build, no timing launch; the slab width, the XCD map and the pacing stay
// (none of them changes a sum).  Validation first: the caller's values and row bounds go to staging buffers that nothing
// else reads.
void Solver::updateMatrix(const double* aValue, int64_t numNz, const pdlp_update_t* u) {
  // on a Hessian-updatable solver this is pdlp_mi355x_update_values without q_value (a NULL a_value stays refused)
  if ((opt_.updatable & PDLP_UPDATABLE_HESSIAN) && !sharded_ && aValue) return updateValues(aValue, numNz, nullptr, 0, u);
  updateMatrixImpl(aValue, numNz, u, nullptr);
}

void Solver::updateMatrixImpl(const double* aValue, int64_t numNz, const pdlp_update_t* u, const double* qValue) {
  const auto t0 = clock::now();
  if (sharded_) refuseSharded(kEntryUpdateMatrix);
  if (!(opt_.updatable & PDLP_UPDATABLE_MATRIX)) refuseNoMatrixBit(kEntryUpdateMatrix);
  if (hasQoff_ && !hessianUpdatable_) refuseOffDiagonalHessian(kEntryUpdateMatrix);
  if (!matrixUpdatable_) throw std::runtime_error("pdlp_mi355x_update_matrix: the solver kept nothing for matrix updates");
  checkMatrixUpdateShape(aValue, numNz, nnzIn_);
  static const pdlp_update_t kNoData{};
  const pdlp_update_t& ud = u ? *u : kNoData;
  checkUpdateShape(ud);
  const int32_t n0 = F_.n0, n = F_.n, m = F_.m;
  const int64_t nnz = F_.nnz, nnz0 = nnzIn_;
  const int32_t mask = updateMask(ud);
  PDLP_HIP(hipSetDevice(opt_.device));
  PDLP_HIP(hipStreamSynchronize(stream_));
  ensureDataStaging();
  if (updMat_.size() == 0) updMat_.alloc((size_t)nnz0);
  const DataStage D = DataStage::over(updIn_.get(), n0, m);
  stagePut(updMat_.get(), aValue, nnz0);
  stageRowsAndValidate(ud, mask, D);
  if (gpuAbsMax(updMat_.get(), nnz0, stream_) == 0.0) throwAllZeroMatrix();  // (a NaN among the values is not zero, as for create)
  if (qValue) stageHessian(qValue);
  // ---- nothing below is refused ----
  stageColumns(ud, mask, D);
  PDLP_HIP(hipStreamSynchronize(stream_));
  updMatSeconds_[kMatStage] = since(t0);

  // formulated values in reference order, their row-major copy through the kept permutation; the unscaled data overlaid
  // with what u gives (the replay kernels with no pass), copied into the solver's vectors
  auto t1 = clock::now();
  MatrixKeep& K = mk_;
  if (qValue) launchHessianAssemble(hk_.dstBeg.get(), hk_.srcSlot.get(), updQ_.get(), F_.sense, n, hk_.nOff, K.qdiag0.get(),
                                    hk_.qoff0.get(), stream_);
  gpuFormulateValues(K.aStart.get(), K.aIndex.get(), updMat_.get(), rowKindDev_.get(), rowNewIdxDev_.get(), n0, m, nnz0, nnz - nnz0,
                     K.cscVal.get(), stream_);
  launchRefill(K.permA.get(), K.cscVal.get(), nnz, nnz, K.aVal.get(), stream_);
  replayData(mask, D, nullptr, nullptr, 0, K.cost0.get(), K.lower0.get(), K.upper0.get(), K.rhs0.get());
  auto copy = [&](double* dst, const double* src, int64_t count) {
    if (count > 0) PDLP_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)count, hipMemcpyDeviceToDevice, stream_));
  };
  copy(cost_.get(), K.cost0.get(), n);
  copy(lower_.get(), K.lower0.get(), n);
  copy(upper_.get(), K.upper0.get(), n);
  copy(rhs_.get(), K.rhs0.get(), m);
  if (qdiag_.size()) copy(qdiag_.get(), K.qdiag0.get(), n);
  gpuFill(colScale_.get(), 1.0, n, stream_);
  gpuFill(rowScale_.get(), 1.0, m, stream_);
  PDLP_HIP(hipStreamSynchronize(stream_));
  updMatSeconds_[kMatFormulate] = since(t1);

  t1 = clock::now();
  if (F_.scaled) {  // (PDLP_FEATURE_SCALING_OFF: nothing is scaled, no pass is kept)
    ScaleOperands o;
    o.n = n; o.m = m; o.nnz = nnz;
    o.cscBeg = K.cscBeg.get(); o.cscIdx = K.cscIdx.get(); o.cscCol = K.cscCol.get(); o.cscVal = K.cscVal.get();
    o.aBeg = K.aBeg.get(); o.aMajor = K.aMajor.get(); o.aIdx = K.aIdx.get(); o.aVal = K.aVal.get();
    o.cost = cost_.get(); o.lower = lower_.get(); o.upper = upper_.get(); o.rhs = rhs_.get();
    o.colScale = colScale_.get(); o.rowScale = rowScale_.get();
    o.qdiag = qdiag_.size() ? qdiag_.get() : nullptr;
    o.csPass = csPass_.get(); o.rsPass = rsPass_.get();  // a later pdlp_mi355x_update replays the NEW factors
    nPass_ = gpuScalePasses(o, stream_);
  }
  updMatSeconds_[kMatPasses] = since(t1);

  // the off-diagonal part of the Hessian through the NEW factors (the diagonal rode along with the passes, as in create)
  if (hessianUpdatable_ && hk_.nOff > 0) applyHessian(false, false);

  t1 = clock::now();
  refillOperands();
  PDLP_HIP(hipStreamSynchronize(stream_));
  updMatSeconds_[kMatRefills] = since(t1);

  // matNormInf, the host copies of the scale vectors, the left-to-right sums of the scaled c, b — as the set-up does;
  // the termination norms are those of the unscaled data and change with u only
  t1 = clock::now();
  F_.matNormInf = gpuAbsMax(K.cscVal.get(), nnz, stream_);
  colScale_.download(F_.colScale.data(), (size_t)n, stream_);
  rowScale_.download(F_.rowScale.data(), (size_t)m, stream_);
  refreshScaledSums(true, true);  // (its synchronisation covers the two downloads above)
  if (mask & kUpdCost) F_.normCost = unscaledNormCost(ud.col_cost, n0, F_.sense);
  if (mask & kUpdRows) F_.normRhs = unscaledNormRhs(ud.row_lower, ud.row_upper, F_.rowKind.data(), m);
  if (ud.has_offset) F_.offset = ud.offset;
  updMatSeconds_[kMatSums] = since(t1);

  t1 = clock::now();
  const bool recapture = fused_ && refreshBoundsFlipsUniform();  // every scaled bound has changed
  updMatSeconds_[kMatBounds] = since(t1);
  finishUpdate(ud, recapture, &updMatSeconds_[kMatReset], &updMatSeconds_[kMatCapture], t0);
}

}  // namespace pdlp
