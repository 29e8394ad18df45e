// pdlp_batch_lanes.cpp — the device side of a batch (pdlp_batch.hpp): Solver's lane steps, i.e. Solver::run cut into the
// pieces the driver calls per lane; the lane and the backend the driver works with on a device; the batch itself.
#include <algorithm>
#include <cstdio>
#include <cstring>

#include "pdlp_batch.hpp"
#include "pdlp_batch_resident.hpp"
#include "pdlp_pool.hpp"
#include "pdlp_resident.hpp"
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

void Solver::laneFinish(pdlp_result_t* R, bool resultOnDevice) {
  if (!loop_.noLoop) endDeviceLoop();
  finishRun(R, resultOnDevice);
}

Solver::VariantCheckFacts Solver::laneVariantCheckFacts() const {
  VariantCheckFacts f;
  if (rowKindDev_.size() == (size_t)F_.m) f.rowKindDev = rowKindDev_.get();
  f.rowKindHost = F_.rowKind.data();
  if (hessianUpdatable_ && hk_.dstBeg.size() > (size_t)F_.n && hk_.nSlots > 0) {
    f.dstBeg = hk_.dstBeg.get();
    f.srcSlot = hk_.srcSlot.get();
  }
  f.sense = F_.sense;
  f.m = F_.m;
  f.n = F_.n;
  f.nnz = nnzIn_;
  return f;
}

namespace {

// What a batch keeps for its device runs (pdlp_mi355x_batch_run_device): P's updatable data in HBM — uploaded by the first
// device run, kept with the batch; what a lane restores in a device call comes from here —, the table and the records of
// the validation launch, and the stream of the call in progress.
struct BatchResident {
  int32_t device = 0;
  const BaseData* base = nullptr;
  std::vector<Solver*> solvers;
  hipStream_t callerStream = nullptr;  // of the call in progress
  DeviceArray<double> baseDev;         // cost, colLower, colUpper, rowLower, rowUpper, aValue, qValue, back to back
  BaseView view;                       // ... as the plan takes it
  bool uploaded = false;
  DeviceArray<VariantJob> jobs;
  DeviceArray<VariantRecord> rec;

  // P's data into HBM, once (on lane 0's stream; synchronises)
  void ensureBase() {
    if (uploaded) return;
    const BaseData& b = *base;
    const std::vector<double>* part[7] = {&b.cost, &b.colLower, &b.colUpper, &b.rowLower, &b.rowUpper, &b.aValue, &b.qValue};
    size_t total = 0;
    for (const auto* p : part) total += p->size();
    baseDev.alloc(total);
    const double* at[7];
    size_t off = 0;
    hipStream_t s = solvers[0]->laneStream();
    for (int i = 0; i < 7; ++i) {
      at[i] = baseDev.get() + off;
      if (!part[i]->empty())
        PDLP_HIP(hipMemcpyAsync(baseDev.get() + off, part[i]->data(), sizeof(double) * part[i]->size(), hipMemcpyHostToDevice, s));
      off += part[i]->size();
    }
    PDLP_HIP(hipStreamSynchronize(s));
    view = b.view();
    view.cost = at[0]; view.colLower = at[1]; view.colUpper = at[2]; view.rowLower = at[3]; view.rowUpper = at[4];
    view.aValue = at[5]; view.qValue = at[6];
    uploaded = true;
  }

  // Refusal step 1 of pdlp_mi355x_batch_run_device: what the entry a variant maps to refuses without looking at a value,
  // from host facts.  No HIP call.
  void refuseValueFree(int32_t K, const Variant* v) const {
    const ValueUpdateFacts f = solvers[0]->valueUpdateFacts();
    for (int32_t k = 0; k < K; ++k) {
      try {
        residentUpdateRefusal(f, v[k].a_value, v[k].num_nz, v[k].q_value, v[k].num_q_nz, v[k].u);
        // updateDevice's own last value-free refusal.  A lane is never sharded and keeps its matrix exactly where the line
        // above lets an a_value pass (the MATRIX bit, and no off-diagonal Hessian without the HESSIAN bit), so this does
        // not fire; it stands here so that nothing an update refuses without looking at a value is left for mid-run.
        if (v[k].a_value && !solvers[0]->laneKeepsMatrix())
          throw std::runtime_error("pdlp_mi355x_update_matrix: the solver kept nothing for matrix updates");
      } catch (const std::exception& e) {
        throw std::runtime_error("variant " + std::to_string(k) + ": " + e.what());
      }
    }
  }
  // Step 2, THE POINTER CHECK (pdlp_resident.hpp): every array of every variant, then every vector of every result.
  // Launches nothing, copies nothing.
  void requirePointers(int32_t K, const Variant* v, const pdlp_result_t* R) const {
    auto named = [&](const char* what, int32_t k, auto&& check) {
      try {
        check();
      } catch (const std::exception& e) {
        throw std::runtime_error(std::string(what) + " " + std::to_string(k) + ": " + e.what());
      }
    };
    for (int32_t k = 0; k < K; ++k) named("variant", k, [&] { requireDeviceUpdate(v[k].a_value, v[k].q_value, &v[k].u, device); });
    if (R)
      for (int32_t k = 0; k < K; ++k) named("result", k, [&] { requireDeviceResult(R[k], device); });
  }
  // Every lane's stream behind ONE event recorded on the caller's stream, which is never synchronised
  void orderLanes() const {
    hipEvent_t ev = nullptr;
    PDLP_HIP(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
    hipError_t e = hipEventRecord(ev, callerStream);
    for (size_t l = 0; l < solvers.size() && e == hipSuccess; ++l) e = hipStreamWaitEvent(solvers[l]->laneStream(), ev, 0);
    (void)hipEventDestroy(ev);  // (released once the waits have passed it)
    PDLP_HIP(e);
  }
  // Step 3's launch on lane 0's stream: nRec >= K records initialised to {m, 0, n}, the K jobs' in ONE launch, all nRec
  // records back in one copy; synchronises.
  std::vector<VariantRecord> records(int32_t K, const Variant* v, int32_t nRec) {
    const Solver::VariantCheckFacts f = solvers[0]->laneVariantCheckFacts();
    hipStream_t s = solvers[0]->laneStream();
    std::vector<VariantJob> table((size_t)K);
    bool rows = false;
    for (int32_t k = 0; k < K; ++k) {
      table[(size_t)k] = VariantJob{v[k].u.row_lower, v[k].u.row_upper, v[k].a_value, v[k].q_value};
      rows = rows || v[k].u.row_lower;
    }
    if (rows && f.m > 0 && !f.rowKindDev) throw std::runtime_error("pdlp_mi355x_batch_run_device: the lanes did not keep their row kinds");
    std::vector<VariantRecord> rec0((size_t)nRec, VariantRecord{f.m, 0, f.n});
    if (jobs.size() < (size_t)K) jobs.alloc((size_t)K);
    if (rec.size() < (size_t)nRec) rec.alloc((size_t)nRec);
    jobs.upload(table.data(), (size_t)K, s);
    rec.upload(rec0.data(), (size_t)nRec, s);
    VariantsValidateArgs a{};
    a.jobs = jobs.get(); a.K = K;
    a.rowKind = f.rowKindDev; a.dstBeg = f.dstBeg; a.srcSlot = f.srcSlot;
    a.sense = f.sense; a.m = f.m; a.n = f.n; a.nnz = f.nnz;
    a.rec = rec.get();
    launchVariantsValidate(a, s);
    rec.download(rec0.data(), (size_t)nRec, s);
    PDLP_HIP(hipStreamSynchronize(s));
    return rec0;
  }
  // The three steps, in their fixed order; all-or-nothing: nothing of a lane is written
  void validate(int32_t K, const Variant* v, const pdlp_result_t* R) {
    refuseValueFree(K, v);
    requirePointers(K, v, R);
    // ---- from here on every pointer is known to be HBM of this device ----
    PDLP_HIP(hipSetDevice(device));
    ensureBase();
    orderLanes();
    const std::vector<VariantRecord> rec0 = records(K, v, K);
    const Solver::VariantCheckFacts f = solvers[0]->laneVariantCheckFacts();
    hipStream_t s = solvers[0]->laneStream();
    refuseByRecords(K, v, rec0.data(), f.rowKindHost, f.m, f.n, [&](int32_t k, int32_t row, double* lo, double* up) {
      PDLP_HIP(hipMemcpyAsync(lo, v[k].u.row_lower + row, sizeof(double), hipMemcpyDeviceToHost, s));  // that row's two bounds only
      PDLP_HIP(hipMemcpyAsync(up, v[k].u.row_upper + row, sizeof(double), hipMemcpyDeviceToHost, s));
      PDLP_HIP(hipStreamSynchronize(s));
    });
  }
};

class SolverLane : public BatchLane {
 public:
  SolverLane(Solver* s, const pdlp_params_t& opt, const BaseData* base, BatchResident* resident)
      : s_(s), opt_(opt), hostView_(base->view()), resident_(resident) {
    tap_.sink = opt.log_callback;
    tap_.sinkCtx = opt.log_ctx;
  }
  void setMode(LaneMode mode) override { mode_ = mode; }
  void validateDevice(int32_t K, const Variant* v, const pdlp_result_t* R) override { resident_->validate(K, v, R); }
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
    const bool dev = mode_ == kLaneDevice;  // (the batch's copy of P in HBM is there: validateDevice has run)
    const LaneUpdatePlan plan = planLaneUpdate(v, differs_, dev ? resident_->view : hostView_);
    const Variant& w = plan.v;
    differs_ |= plan.now;  // (also when the update throws half-way: a needless restore costs time only)
    // (device: ONE entry routes the three updates as the plan does; the lane's stream is ordered behind the caller's already)
    if (dev) s_->updateDeviceBehind(w.a_value, w.num_nz, w.q_value, w.num_q_nz, &w.u, resident_->callerStream, false);
    else if (plan.call == kCallUpdate) s_->update(w.u);
    else if (plan.call == kCallUpdateMatrix) s_->updateMatrix(w.a_value, w.num_nz, &w.u);
    else s_->updateValues(w.a_value, w.num_nz, w.q_value, w.num_q_nz, &w.u);
    differs_ = plan.now;
  }
  void runAlone(pdlp_result_t* R) override {
    if (mode_ == kLaneDevice) s_->runDevice(R);
    else s_->run(R);
  }
  void begin() override { s_->laneBegin(); }
  bool idle() override { return s_->laneIdle(); }
  void queue(int32_t ahead, std::vector<LaneUnit>& units) override { s_->laneQueue(ahead, units); }
  LaneVerdict afterRound() override { return s_->laneAfterRound(); }
  void finish(pdlp_result_t* R) override { s_->laneFinish(R, mode_ == kLaneDevice); }
  int32_t xcc() override { return s_->laneXcc(); }

 private:
  Solver* s_;
  pdlp_params_t opt_;
  BaseView hostView_;  // P's data where a host call restores from (the batch keeps the vectors)
  BatchResident* resident_;
  LaneMode mode_ = kLaneHost;  // of the call in progress
  int differs_ = 0;  // the arrays in which the solver's problem differs from P (wherever the arrays came from)
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

std::string batchVariantDeviceRefusal(const pdlp_problem_t& P, const pdlp_params_t& opt, const Variant& v) {
  try {
    const SessionShape shape = sessionShapeOf(P);
    ValueUpdateFacts f;  // (as above; no kinds: residentUpdateRefusal leaves them to the device)
    f.updatable = opt.updatable | PDLP_UPDATABLE_DATA;
    f.nnz = shape.nnz;
    f.qSlots = (opt.updatable & PDLP_UPDATABLE_HESSIAN) ? shape.qSlots : 0;
    f.hasQoff = (opt.updatable & PDLP_UPDATABLE_HESSIAN) ? hessianHasOffDiagonalSlot(P) : hessianHasOffDiagonal(P);
    residentUpdateRefusal(f, v.a_value, v.num_nz, v.q_value, v.num_q_nz, v.u);
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
  BatchResident resident;
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
  impl_->resident.device = o.device;
  impl_->resident.base = impl_->base.get();
  std::vector<BatchLane*> ls;
  std::vector<Solver*> ss;
  for (int32_t l = 0; l < lanes; ++l) {
    impl_->solvers.emplace_back(new Solver(P, o, 0, 1, nullptr));
    impl_->lanes.emplace_back(new SolverLane(impl_->solvers.back().get(), o, impl_->base.get(), &impl_->resident));
    ls.push_back(impl_->lanes.back().get());
    ss.push_back(impl_->solvers.back().get());
  }
  impl_->resident.solvers = ss;
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

void Batch::runDevice(int32_t K, const Variant* vDev, pdlp_result_t* RDev, hipStream_t callerStream) {
  // (no HIP call here: the refusals that need none come first, inside the driver's validation — BatchResident::validate)
  impl_->resident.callerStream = callerStream;
  driver_->run(K, vDev, RDev, kEntryBatchRunDevice, kLaneDevice);
}

void Batch::variantRecords(int32_t K, const Variant* vDev, int32_t nRec, int32_t* out) {
  refuseBatchArguments("pdlp_mi355x_batch_variant_records", K, vDev, out);
  if (nRec < K) throw std::runtime_error("pdlp_mi355x_batch_variant_records: fewer records than variants");
  BatchResident& r = impl_->resident;
  r.refuseValueFree(K, vDev);
  r.requirePointers(K, vDev, nullptr);
  PDLP_HIP(hipSetDevice(impl_->device));
  r.callerStream = nullptr;
  r.orderLanes();
  const std::vector<VariantRecord> rec = r.records(K, vDev, nRec);
  static_assert(sizeof(VariantRecord) == 3 * sizeof(int32_t), "three int32 per record");
  memcpy(out, rec.data(), sizeof(VariantRecord) * (size_t)nRec);
}

}  // namespace pdlp
