// pdlp_resident.cpp — the host side of the device-resident entries (see pdlp_resident.hpp): the pointer check, the host
// shadow of a problem in HBM, Solver::updateDevice / runDevice / postsolveDevice.
#include "pdlp_resident.hpp"

#include <chrono>
#include <cstring>
#include <stdexcept>
#include <string>

#include "pdlp_solver.hpp"

namespace pdlp {

// ---- the pointer check ------------------------------------------------------------------------------------------------
void requireDevicePointer(const void* p, const char* field, int device) {
  if (!p) return;
  hipPointerAttribute_t a;
  memset(&a, 0, sizeof(a));
  const hipError_t e = hipPointerGetAttributes(&a, p);
  bool ok = e == hipSuccess && a.type == hipMemoryTypeDevice && !a.isManaged && a.device == device;
  if (e != hipSuccess) (void)hipGetLastError();  // (a pointer the runtime does not know: the error would stick otherwise)
  if (!ok) throw std::runtime_error(std::string(field) + " is not device memory on device " + std::to_string(device));
}

void requireDeviceProblem(const pdlp_problem_t& P, int device) {
  requireDevicePointer(P.a_start, "a_start", device);
  requireDevicePointer(P.a_index, "a_index", device);
  requireDevicePointer(P.a_value, "a_value", device);
  requireDevicePointer(P.col_cost, "col_cost", device);
  requireDevicePointer(P.col_lower, "col_lower", device);
  requireDevicePointer(P.col_upper, "col_upper", device);
  requireDevicePointer(P.row_lower, "row_lower", device);
  requireDevicePointer(P.row_upper, "row_upper", device);
  requireDevicePointer(P.start_col_value, "start_col_value", device);
  requireDevicePointer(P.start_row_value, "start_row_value", device);
  requireDevicePointer(P.start_row_dual, "start_row_dual", device);
  requireDevicePointer(P.q_start, "q_start", device);
  requireDevicePointer(P.q_index, "q_index", device);
  requireDevicePointer(P.q_value, "q_value", device);
}

void requireDeviceUpdate(const double* aValue, const double* qValue, const pdlp_update_t* u, int device) {
  requireDevicePointer(aValue, "a_value", device);
  requireDevicePointer(qValue, "q_value", device);
  if (!u) return;
  requireDevicePointer(u->col_cost, "col_cost", device);
  requireDevicePointer(u->col_lower, "col_lower", device);
  requireDevicePointer(u->col_upper, "col_upper", device);
  requireDevicePointer(u->row_lower, "row_lower", device);
  requireDevicePointer(u->row_upper, "row_upper", device);
  requireDevicePointer(u->start_col_value, "start_col_value", device);
  requireDevicePointer(u->start_row_value, "start_row_value", device);
  requireDevicePointer(u->start_row_dual, "start_row_dual", device);
}

void requireDeviceResult(const pdlp_result_t& R, int device) {
  requireDevicePointer(R.col_value, "col_value", device);
  requireDevicePointer(R.col_dual, "col_dual", device);
  requireDevicePointer(R.row_value, "row_value", device);
  requireDevicePointer(R.row_dual, "row_dual", device);
}

void orderBehind(hipStream_t s, hipStream_t caller) {
  hipEvent_t ev = nullptr;
  PDLP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
  hipError_t e = hipEventRecord(ev, caller);
  if (e == hipSuccess) e = hipStreamWaitEvent(s, ev, 0);
  (void)hipEventDestroy(ev);  // (released once the wait has passed it)
  PDLP_HIP(e);
}

// ---- create_device ----------------------------------------------------------------------------------------------------
void residentProblemShape(const pdlp_problem_t& P) {
  if (P.num_col < 0 || P.num_row < 0) throw std::runtime_error("negative dimensions");
  if (P.num_col > 0 && (!P.a_start || !P.col_cost || !P.col_lower || !P.col_upper)) throw std::runtime_error("null column arrays");
  if (P.num_row > 0 && (!P.row_lower || !P.row_upper)) throw std::runtime_error("null row arrays");
  if (P.num_nz > 0 && (!P.a_index || !P.a_value)) throw std::runtime_error("null matrix arrays");
}

ResidentProblem::ResidentProblem(const pdlp_problem_t& Pdev, hipStream_t caller) : shadow(Pdev), callerStream(caller) {
  in.aStart = Pdev.a_start; in.aIndex = Pdev.a_index; in.aValue = Pdev.a_value;
  in.colCost = Pdev.col_cost; in.colLower = Pdev.col_lower; in.colUpper = Pdev.col_upper;
  in.rowLower = Pdev.row_lower; in.rowUpper = Pdev.row_upper;
  hess.qStart = Pdev.q_start; hess.qIndex = Pdev.q_index; hess.qValue = Pdev.q_value;
  if (Pdev.q_dim > 0 && Pdev.q_start) in.hessian = &hess;
}

void ResidentProblem::fetchShadow(hipStream_t s) {
  orderBehind(s, callerStream);
  const size_t n0 = (size_t)std::max(shadow.num_col, 0), m = (size_t)std::max(shadow.num_row, 0);
  auto pull = [&](auto& host, const auto* dev, size_t count) {
    host.resize(count);
    if (count > 0) PDLP_HIP(hipMemcpyAsync(host.data(), dev, sizeof(*dev) * count, hipMemcpyDeviceToHost, s));
  };
  if (n0 > 0) {
    pull(hStart, in.aStart, n0 + 1);
    pull(hCost, in.colCost, n0);
  }
  if (m > 0) {
    pull(hRowLower, in.rowLower, m);
    pull(hRowUpper, in.rowUpper, m);
  }
  const bool qp = shadow.q_dim > 0 && shadow.q_start;
  if (qp) pull(hQStart, hess.qStart, (size_t)shadow.q_dim + 1);
  const bool hot = shadow.start_value_valid && shadow.start_dual_valid && shadow.start_col_value && shadow.start_row_value &&
                   shadow.start_row_dual;
  if (hot) {
    pull(hStartCol, shadow.start_col_value, n0);
    pull(hStartRow, shadow.start_row_value, m);
    pull(hStartDual, shadow.start_row_dual, m);
  }
  PDLP_HIP(hipStreamSynchronize(s));
  if (n0 > 0) { shadow.a_start = hStart.data(); shadow.col_cost = hCost.data(); }
  if (m > 0) { shadow.row_lower = hRowLower.data(); shadow.row_upper = hRowUpper.data(); }
  if (qp) shadow.q_start = hQStart.data();
  if (hot) {
    shadow.start_col_value = hStartCol.data(); shadow.start_row_value = hStartRow.data(); shadow.start_row_dual = hStartDual.data();
  } else {  // (a start the host entry would not use either)
    shadow.start_col_value = shadow.start_row_value = shadow.start_row_dual = nullptr;
  }
}

bool ResidentProblem::hasOffDiagonalHessian(bool everySlot, bool switchOn, hipStream_t s) {
  const pdlp_problem_t& P = shadow;
  const int32_t reason = hessianExtractionReason(true, false, false, switchOn, P.q_dim, P.q_start);
  if (reason == kHessNoSlots) return false;
  if (reason == kHessStarts)
    throw std::runtime_error("q_start does not run from 0 without decreasing: only the host walk defines what that means, and it "
                             "needs the Hessian in host memory (pdlp_mi355x_create)");
  if (reason != kHessOnDevice)
    throw std::runtime_error("PDLP_MI355X_GPU_HESSIAN=0 asks for the host walk, which needs the Hessian in host memory "
                             "(pdlp_mi355x_create)");
  if (P.q_dim > P.num_col) throw std::runtime_error("Hessian dimension exceeds the number of columns");
  if (!P.q_index || !P.q_value) throw std::runtime_error("null Hessian arrays");
  return gpuHessianHasOffDiagonal(hess.qStart, hess.qIndex, hess.qValue, P.q_dim, everySlot, s);
}

// ---- update_device ----------------------------------------------------------------------------------------------------
ResidentRoute residentRoute(int32_t updatable, const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz) {
  if (!aValue && !qValue && numNz == 0 && numQNz == 0) return kRouteUpdate;
  if (aValue && !qValue && numQNz == 0 && !(updatable & PDLP_UPDATABLE_HESSIAN)) return kRouteUpdateMatrix;
  return kRouteUpdateValues;
}

void residentUpdateRefusal(const ValueUpdateFacts& f, const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz,
                           const pdlp_update_t& u) {
  ValueUpdateFacts g = f;
  g.rowKind = nullptr;  // (the row bounds are in HBM: the kinds are compared there, by the update's validation kernel)
  g.m = 0;
  if (residentRoute(f.updatable, aValue, numNz, qValue, numQNz) == kRouteUpdate) {
    if (g.sharded) refuseSharded(kEntryUpdate);
    if (!g.updatable) refuseNotUpdatable(kEntryUpdate);
    checkUpdateShape(u);
    return;
  }
  refuseValueUpdate(g, aValue, numNz, qValue, numQNz, u);
}

void SolverBase::runDevice(pdlp_result_t*) {
  throw std::runtime_error("HiPDLP solvers (algorithm = 1) do not take updates");  // (sessionOneShotReason's words)
}
void SolverBase::updateDevice(const double*, int64_t, const double*, int64_t, const pdlp_update_t*, hipStream_t) {
  throw std::runtime_error("HiPDLP solvers (algorithm = 1) do not take updates");
}

// The three updates with the caller's arrays in HBM.  What the host entries refuse without looking at a value is refused
// first, from host facts; then the pointer check; then the arrays go device to device into the staging buffers the host
// entries upload into (nothing of the solver's problem), and the host entry runs from there as it does for a session —
// with downloaded copies of the arrays it reads on the host (costs and row bounds for the norms and the kind-change
// message, a hot start), and the caller's pointers for those it only asks about (never read: staged_).
void Solver::updateDevice(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u,
                          hipStream_t callerStream) {
  updateDeviceBehind(aValue, numNz, qValue, numQNz, u, callerStream, true);
}

void Solver::updateDeviceBehind(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u,
                                hipStream_t callerStream, bool order) {
  const auto t0 = std::chrono::steady_clock::now();
  static const pdlp_update_t kNoData{};
  const pdlp_update_t& ud = u ? *u : kNoData;
  const ValueUpdateFacts f = valueUpdateFacts();  // (as a batch's validation takes them; the kinds are left to the device)
  const ResidentRoute route = residentRoute(opt_.updatable, aValue, numNz, qValue, numQNz);
  if (route == kRouteUpdate && !u) throw std::runtime_error("pdlp_mi355x_update: null update");
  residentUpdateRefusal(f, aValue, numNz, qValue, numQNz, ud);
  if (aValue && !matrixUpdatable_) throw std::runtime_error("pdlp_mi355x_update_matrix: the solver kept nothing for matrix updates");
  requireDeviceUpdate(aValue, qValue, u, opt_.device);

  // ---- the first copy: from here on every pointer is known to be HBM of this device ----
  const int32_t n0 = F_.n0, m = F_.m;
  const int32_t mask = updateMask(ud);
  PDLP_HIP(hipSetDevice(opt_.device));
  PDLP_HIP(hipStreamSynchronize(stream_));
  if (order) orderBehind(stream_, callerStream);
  std::vector<double> hCost, hRowLower, hRowUpper, hStartCol, hStartRow, hStartDual;
  auto pull = [&](std::vector<double>& host, const double* dev, size_t count) {
    host.resize(count);
    if (count > 0) PDLP_HIP(hipMemcpyAsync(host.data(), dev, sizeof(double) * count, hipMemcpyDeviceToHost, stream_));
  };
  auto stage = [&](double* dst, const double* src, int64_t count) {
    if (count > 0) PDLP_HIP(hipMemcpyAsync(dst, src, sizeof(double) * (size_t)count, hipMemcpyDeviceToDevice, stream_));
  };
  ensureDataStaging();
  const DataStage D = DataStage::over(updIn_.get(), n0, m);
  pdlp_update_t uh = ud;
  if (mask & kUpdCost) { pull(hCost, ud.col_cost, (size_t)n0); stage(D.cost, ud.col_cost, n0); uh.col_cost = hCost.data(); }
  if (mask & kUpdColLower) stage(D.colLower, ud.col_lower, n0);
  if (mask & kUpdColUpper) stage(D.colUpper, ud.col_upper, n0);
  if (mask & kUpdRows) {
    pull(hRowLower, ud.row_lower, (size_t)m); pull(hRowUpper, ud.row_upper, (size_t)m);
    stage(D.rowLower, ud.row_lower, m); stage(D.rowUpper, ud.row_upper, m);
    uh.row_lower = hRowLower.data(); uh.row_upper = hRowUpper.data();
  }
  if (ud.start_col_value) {
    pull(hStartCol, ud.start_col_value, (size_t)n0); pull(hStartRow, ud.start_row_value, (size_t)m);
    pull(hStartDual, ud.start_row_dual, (size_t)m);
    uh.start_col_value = hStartCol.data(); uh.start_row_value = hStartRow.data(); uh.start_row_dual = hStartDual.data();
  }
  if (aValue) {
    if (updMat_.size() == 0) updMat_.alloc((size_t)nnzIn_);
    stage(updMat_.get(), aValue, nnzIn_);
  }
  if (qValue) {
    if (updQ_.size() == 0) updQ_.alloc((size_t)hk_.nSlots);
    stage(updQ_.get(), qValue, hk_.nSlots);
  }
  PDLP_HIP(hipStreamSynchronize(stream_));  // the shadows are read on the host below; the caller's arrays are free again

  struct Staged {  // (as a session sets it: the entries below take the arrays from the staging buffers)
    bool& flag;
    const bool was;
    explicit Staged(bool& f_) : flag(f_), was(f_) { flag = true; }
    ~Staged() { flag = was; }
  } staged(staged_);
  const double before = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  if (route == kRouteUpdate) update(uh);
  else if (route == kRouteUpdateMatrix) updateMatrix(aValue, numNz, u ? &uh : nullptr);
  else updateValues(aValue, numNz, qValue, numQNz, u ? &uh : nullptr);
  // the update's time (setup_seconds of the next run) and its staging part include the check, the downloads and the copies
  setupSeconds_ += before;
  (aValue ? updMatSeconds_[kMatStage] : updSeconds_[kUpdStage]) += before;
}

// ---- run_device -------------------------------------------------------------------------------------------------------
void Solver::runDevice(pdlp_result_t* R) {
  if (sharded_) throw std::runtime_error("sharded solvers (pdlp_mi355x_create_sharded) do not take updates");
  if (R) requireDeviceResult(*R, opt_.device);
  PDLP_HIP(hipSetDevice(opt_.device));  // (the first run_device allocates the post-solve's row bookkeeping)
  reset();
  solveBeg_ = std::chrono::steady_clock::now();
  if (hasStart_) log(1, "Hot starting with given column primal values and row dual values\n");
  if (devCheck_ && !profile_) doSolveDevice(true, 0);
  else doSolve(true, 0);
  finishRun(R, true);
}

// PDHG_PostSolve as Solver::postsolve does it, on the solver's stream; the results are complete on return
void Solver::postsolveDevice(pdlp_result_t* R) {
  const int32_t n0 = F_.n0, m = F_.m;
  const bool useAvg = (termCode_ == PDLP_TERM_OPTIMAL && termIterate_ == 1);
  const int c = hostState_->cur;
  // first run_device: the row bookkeeping the kernels read.  An updatable solver holds kinds and permutation in HBM already
  // (keepForUpdates); the rank is the exclusive count of the ranged-or-free rows — row i's slack column is n0 + rank[i] —
  // taken once from the host's copy of the kinds (the set-up's own scan of them is a temporary of gpuPrepare)
  const bool ownRows = rowKindDev_.size() != (size_t)m || rowNewIdxDev_.size() != (size_t)m;
  if (postRank_.size() == 0 && m > 0) {
    std::vector<int32_t> rank((size_t)m);
    int32_t count = 0;
    for (int32_t i = 0; i < m; ++i) { rank[(size_t)i] = count; count += F_.rowKind[(size_t)i] == kRowBound ? 1 : 0; }
    postRank_.alloc((size_t)m);
    postRank_.upload(rank.data(), (size_t)m, stream_);
    if (ownRows) {
      postKind_.alloc((size_t)m); postNewIdx_.alloc((size_t)m);
      postKind_.upload(F_.rowKind.data(), (size_t)m, stream_);
      postNewIdx_.upload(F_.rowNewIdx.data(), (size_t)m, stream_);
    }
    PDLP_HIP(hipStreamSynchronize(stream_));  // (rank goes out of scope)
  }
  PostsolveArgs a{};
  a.x = (useAvg ? xAvg_ : x_[c]).get();
  a.slackPos = (useAvg ? slackPosAvg_ : slackPos_).get();
  a.slackNeg = (useAvg ? slackNegAvg_ : slackNeg_).get();
  a.y = useAvg ? yAvgl() : yl(c);
  a.ax = (useAvg ? axAvg_ : ax_[c]).get();
  a.colScale = colScale_.get(); a.rowScale = rowScale_.get();
  a.rowKind = ownRows ? postKind_.get() : rowKindDev_.get();
  a.rowNewIdx = ownRows ? postNewIdx_.get() : rowNewIdxDev_.get();
  a.rowRank = postRank_.get();
  a.n0 = n0; a.m = m; a.scaled = F_.scaled ? 1 : 0;
  a.sense = F_.sense;
  a.colValue = R->col_value; a.colDual = R->col_dual; a.rowValue = R->row_value; a.rowDual = R->row_dual;
  launchPostsolve(a, stream_);
  PDLP_HIP(hipStreamSynchronize(stream_));
  postsolveScalars(R, R->col_value != nullptr, R->col_dual != nullptr, R->row_value != nullptr, R->row_dual != nullptr);
}

}  // namespace pdlp
