// pdlp_batch_lanes.cpp — the device side of a batch (pdlp_batch.hpp): Solver's lane steps, i.e. Solver::run cut into the
// pieces the driver calls per lane; the lane and the backend the driver works with on a device; the batch itself.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "pdlp_batch.hpp"
#include "pdlp_pool.hpp"
#include "pdlp_session.hpp"
#include "pdlp_solver.hpp"
#include "pdlp_update.hpp"

namespace pdlp {

// ---- Solver: one run as a lane ------------------------------------------------------------------------------------------
std::string Solver::laneSequentialReason() const {
  const std::string blocks = std::to_string(smallGrid_) + " work blocks";
  if (sharded_) return "sharded solver";
  if (!persistent_ && hasQoff_ && qpNotPersistent_)
    return std::string("the trial loop is not one persistent launch (off-diagonal Hessian: ") + qpNotPersistent_ + ")";
  if (!persistent_) return "the trial loop is not one persistent launch (" + std::to_string(std::max(dA_.nBlocks, dAt_.nBlocks)) + " work blocks)";
  if (!xcdLocal_) {
    if (smallGrid_ > 32) return blocks + " need more than one XCD";
    if (sw_.xcdLocal == 0) return blocks + ", but the XCD-local mode is switched off";
    return blocks + ", but the XCD-local placement does not hold on this device";
  }
  if (!checkSmall_) return blocks + ", but the check is not one launch";
  if (!devCheck_) return blocks + ", but the checks are driven by the host";
  if (profile_) return blocks + ", but the solver is in profile mode";
  const MatView* nv = hasQoff_ ? &smallQp()->N : nullptr;
  if (!smallLanesSupported(dA_.view(), dAt_.view(), primalInA_, nv) || !checkLanesSupported(dA_.view(), dAt_.view(), nv))
    return blocks + ", but not in 512-entry blocks";
  return std::string();
}

void Solver::validateUpdate(const pdlp_update_t& u) const {
  if (sharded_) refuseSharded(kEntryUpdate);
  if (!updatable_) refuseNotUpdatable(kEntryUpdate);
  checkUpdateShape(u);
  // (the rule of the device's validation kernel, on the host's copy of the kinds)
  if (u.row_lower) refuseKindChange(F_.rowKind.data(), F_.m, u.row_lower, u.row_upper);
}

// The refusals of updateValues / updateMatrix for these arguments, in their order and words.  Those that look at no value
// first (refuseValueUpdate); then the all-zero matrix by the host's rule on the caller's array, and the negative diagonal
// by the update's own head (the assembly map lives on the device only): stageHessian writes the staging copy of q_value
// and the validation kernel's word, which nothing but an update's head reads — nothing of the solver's problem.
ValueUpdateFacts Solver::valueUpdateFacts() const {
  ValueUpdateFacts f;
  f.sharded = sharded_;
  f.updatable = opt_.updatable;
  f.nnz = nnzIn_;
  f.qSlots = hk_.nSlots;
  f.hasQoff = hasQoff_;
  f.rowKind = F_.rowKind.data();
  f.m = F_.m;
  return f;
}

void Solver::validateValues(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t& u) const {
  const ValueUpdateFacts f = valueUpdateFacts();
  refuseValueUpdate(f, aValue, numNz, qValue, numQNz, u);
  if (aValue) {
    bool anyNonzero = false;  // (a NaN among the values is not zero, as for create and for the device's absolute maximum)
    for (int64_t p = 0; p < nnzIn_ && !anyNonzero; ++p) anyNonzero = aValue[p] != 0.0;
    if (!anyNonzero) throwAllZeroMatrix();
  }
  if (qValue) {
    Solver* self = const_cast<Solver*>(this);  // (staging only, see above)
    PDLP_HIP(hipSetDevice(opt_.device));
    PDLP_HIP(hipStreamSynchronize(stream_));
    self->ensureDataStaging();
    self->stageHessian(qValue);
  }
}

// run() up to the first round of its device-driven loop
void Solver::laneBegin() {
  reset();
  solveBeg_ = std::chrono::steady_clock::now();
  if (hasStart_) log(1, "Hot starting with given column primal values and row dual values\n");
  if (!beginDeviceLoop(true, (int64_t)opt_.iter_limit)) return;
  PDLP_HIP(hipStreamSynchronize(stream_));  // (only a lane: the round's launches come on another stream, the batch's)
}

// The units of the next round as launch records (a solver alone launches the same records itself: doSolveDevice)
void Solver::laneQueue(int32_t ahead, std::vector<LaneUnit>& units) {
  const RoundPlan plan = beginRound(ahead);
  if (plan.entryCheck) {
    LaneUnit e;
    e.check = checkSmallLaunch();
    units.push_back(e);
  }
  for (int32_t u = 0; u < plan.nTodo; ++u) {
    LaneUnit unit;
    unit.hasTrials = true;
    unit.trials = smallTrialsLaunch(plan.todo[u] + kRoundSpareTrials);
    unit.check = checkSmallLaunch();
    units.push_back(unit);
  }
}

void Solver::laneDownload(hipStream_t shared) {
  PDLP_HIP(hipMemcpyAsync(hostState_, dst(), sizeof(DevState), hipMemcpyDeviceToHost, shared));
}

// syncState (the stream is idle, the state record is here) + the round's verdict
LaneVerdict Solver::laneAfterRound() {
  DevState& s = *hostState_;
  // Only a lane, and before anything else: a commError is its driver's to handle (a solver alone takes its fall-backs
  // inside syncState).  2: placement, 3: roll call (the launch changed nothing for this lane); 1: barrier timeout (the lane is stopped)
  if (s.commError) {
    loop_.commError = s.commError;
    log(1, "Note: this lane's workgroups of a shared launch %s; its variant is solved alone\n",
        s.commError == 2 ? "were not placed on one XCD" : s.commError == 3 ? "were not resident together in time" : "did not meet at a barrier in time");
    return kLaneFailed;
  }
  // (only a lane: the next launches come on another stream, so refreshed powers are waited for)
  return afterRound(true) ? kLaneGoOn : kLaneOver;
}

int32_t Solver::laneXcc() {
  if (!persistent_ || gridBar_.size() == 0) return -1;
  unsigned long long id = 0;  // (the XCC ids behind the arrival words and the flag: id + 1, 0 = never published)
  PDLP_HIP(hipMemcpyAsync(&id, gridBar_.get() + smallGrid_ + 8, sizeof(id), hipMemcpyDeviceToHost, stream_));
  PDLP_HIP(hipStreamSynchronize(stream_));
  return id == 0 ? -1 : (int32_t)id - 1;
}

void Solver::laneFinish(pdlp_result_t* R) {
  if (!loop_.noLoop) endDeviceLoop();
  finishRun(R);
}

namespace {

class SolverLane : public BatchLane {
 public:
  SolverLane(Solver* s, const pdlp_params_t& opt, const BaseData* base) : s_(s), opt_(opt), base_(base) {
    tap_.sink = opt.log_callback;
    tap_.sinkCtx = opt.log_ctx;
  }
  std::string sequentialReason() override { return s_->laneSequentialReason(); }
  int32_t workBlocks() override { return s_->laneWorkBlocks(); }
  void validate(const Variant& v) override {
    if (!hasValues(v)) s_->validateUpdate(v.u);
    else s_->validateValues(v.a_value, v.num_nz, v.q_value, v.num_q_nz, v.u);
  }
  void setVariant(int32_t k, int32_t iterLimit) override {
    pdlp_params_t o = opt_;
    if (iterLimit > 0) o.iter_limit = iterLimit;
    if (o.log_level >= 1) {
      tap_.prefix = "[variant " + std::to_string(k) + "] ";
      tap_.lineStart = true;
      o.log_callback = &LogTap::write;
      o.log_ctx = &tap_;
    }
    s_->setRuntimeOptions(o);
  }
  void update(const Variant& v) override {
    const LaneUpdatePlan plan = planLaneUpdate(v, differs_, *base_);
    const Variant& w = plan.v;
    differs_ |= plan.now;  // (also when the update throws half-way: a needless restore costs time only)
    if (plan.call == kCallUpdate) s_->update(w.u);
    else if (plan.call == kCallUpdateMatrix) s_->updateMatrix(w.a_value, w.num_nz, &w.u);
    else s_->updateValues(w.a_value, w.num_nz, w.q_value, w.num_q_nz, &w.u);
    differs_ = plan.now;
  }
  void runAlone(pdlp_result_t* R) override { s_->run(R); }
  void begin() override { s_->laneBegin(); }
  bool idle() override { return s_->laneIdle(); }
  void queue(int32_t ahead, std::vector<LaneUnit>& units) override { s_->laneQueue(ahead, units); }
  LaneVerdict afterRound() override { return s_->laneAfterRound(); }
  void finish(pdlp_result_t* R) override { s_->laneFinish(R); }
  int32_t xcc() override { return s_->laneXcc(); }

 private:
  Solver* s_;
  pdlp_params_t opt_;
  const BaseData* base_;
  int differs_ = 0;  // the arrays in which the solver's problem differs from P
  LogTap tap_;
};

// The rounds on the device: LaneRounds (pdlp_pool.hpp) on lane 0's stream, behind the gate of lane 0's device.
class DeviceBackend : public BatchBackend {
 public:
  DeviceBackend(std::vector<Solver*> solvers, int32_t device)
      : solvers_(std::move(solvers)), device_(device), rounds_("pdlp_mi355x_batch_run") {}
  void round(const std::vector<LaneUnit>* units, int nLanes, int32_t* trialLaunches, int32_t* checkLaunches) override {
    int32_t mixed = 0;  // (one problem: never)
    rounds_.round(units, solvers_.data(), nLanes, device_, solvers_[0]->laneStream(), trialLaunches, checkLaunches, &mixed);
  }

 private:
  std::vector<Solver*> solvers_;
  int32_t device_;
  LaneRounds rounds_;
};

}  // namespace

std::string batchCreateRefusal(const pdlp_params_t& opt, int32_t lanes) {
  if (lanes < 1 || lanes > kBatchLanes)
    return "pdlp_mi355x_batch_create: lanes = " + std::to_string(lanes) + " is outside 1..8 (one lane per XCD)";
  if (opt.algorithm != 0 && opt.algorithm != 1) return "unknown algorithm (0 = cuPDLP-C path, 1 = HiPDLP path)";
  if (const char* why = sessionOneShotReason(opt)) return std::string("pdlp_mi355x_batch_create: ") + why;
  return std::string();
}

std::string batchVariantRefusal(const pdlp_problem_t& P, const pdlp_params_t& opt, const Variant& v) {
  try {
    std::vector<int32_t> kind((size_t)std::max(P.num_row, 0));
    for (int32_t i = 0; i < P.num_row; ++i) kind[(size_t)i] = rowKindOf(P.row_lower[i], P.row_upper[i]);
    if (!hasValues(v)) {  // Solver::validateUpdate, on a solver the batch has made updatable
      checkUpdateShape(v.u);
      if (v.u.row_lower) refuseKindChange(kind.data(), P.num_row, v.u.row_lower, v.u.row_upper);
      return std::string();
    }
    const SessionShape shape = sessionShapeOf(P);
    ValueUpdateFacts f;
    f.updatable = opt.updatable | PDLP_UPDATABLE_DATA;
    f.nnz = shape.nnz;
    f.qSlots = (opt.updatable & PDLP_UPDATABLE_HESSIAN) ? shape.qSlots : 0;
    f.hasQoff = (opt.updatable & PDLP_UPDATABLE_HESSIAN) ? hessianHasOffDiagonalSlot(P) : hessianHasOffDiagonal(P);
    f.rowKind = kind.data();
    f.m = P.num_row;
    refuseValueUpdate(f, v.a_value, v.num_nz, v.q_value, v.num_q_nz, v.u);
  } catch (const std::exception& e) {
    return e.what();
  }
  return std::string();
}

struct Batch::Impl {
  std::vector<std::unique_ptr<Solver>> solvers;
  std::vector<std::unique_ptr<SolverLane>> lanes;
  std::unique_ptr<DeviceBackend> backend;
  std::unique_ptr<BaseData> base;
  int32_t device = 0;
};

Batch::Batch(const pdlp_problem_t& P, const pdlp_params_t& opt, int32_t lanes) : impl_(new Impl) {
  const std::string refused = batchCreateRefusal(opt, lanes);
  if (!refused.empty()) throw std::runtime_error(refused);
  pdlp_params_t o = opt;
  o.updatable |= PDLP_UPDATABLE_DATA;
  impl_->device = o.device;
  validateProblem(P);
  impl_->base.reset(new BaseData(P));
  std::vector<BatchLane*> ls;
  std::vector<Solver*> ss;
  for (int32_t l = 0; l < lanes; ++l) {
    impl_->solvers.emplace_back(new Solver(P, o, 0, 1, nullptr));
    impl_->lanes.emplace_back(new SolverLane(impl_->solvers.back().get(), o, impl_->base.get()));
    ls.push_back(impl_->lanes.back().get());
    ss.push_back(impl_->solvers.back().get());
  }
  impl_->backend.reset(new DeviceBackend(ss, o.device));
  driver_.reset(new BatchDriver(ls, impl_->backend.get()));
}

Batch::~Batch() = default;

void Batch::run(int32_t K, const pdlp_update_t* u, pdlp_result_t* R) {
  PDLP_HIP(hipSetDevice(impl_->device));
  std::vector<Variant> v;  // each update as a variant without values
  if (K >= 1 && u) {
    v.resize((size_t)K);
    for (int32_t k = 0; k < K; ++k) {
      memset(&v[(size_t)k], 0, sizeof(Variant));
      v[(size_t)k].u = u[k];
    }
  }
  driver_->run(K, u ? v.data() : nullptr, R, kEntryBatchRun);
}

void Batch::runValues(int32_t K, const Variant* v, pdlp_result_t* R) {
  PDLP_HIP(hipSetDevice(impl_->device));
  driver_->run(K, v, R, kEntryBatchRunValues);
}

}  // namespace pdlp
