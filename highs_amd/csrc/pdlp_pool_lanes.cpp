// pdlp_pool_lanes.cpp — the device side of a pool (pdlp_pool.hpp): the round of shared launches on a caller's stream (also
// the batch's), the lane and the backend the pool driver works with on a device, and the call behind the C ABI.
#include <algorithm>
#include <chrono>
#include <climits>
#include <cstdio>
#include <cstring>

#include "pdlp_pool.hpp"
#include "pdlp_session.hpp"
#include "pdlp_solver.hpp"

namespace pdlp {

// ---- one round of shared launches ---------------------------------------------------------------------------------------
// Everything of a round goes to ONE stream, behind one take of the device gate; the argument records of all its launches
// are written into pinned host memory first and reach HBM in one copy.
LaneRounds::LaneRounds(const char* who) : who_(who) {
  slotT_ = smallLanesSlotBytes();
  slotC_ = checkLanesSlotBytes();
  const size_t bytes = (size_t)kMaxUnits * (slotT_ + slotC_);
  PDLP_HIP(hipHostMalloc(&host_, bytes, hipHostMallocDefault));
  if (hipMalloc(&dev_, bytes) != hipSuccess) {
    (void)hipHostFree(host_);
    throw std::runtime_error(who_ + ": no device memory for the argument records of a round");
  }
}

LaneRounds::~LaneRounds() {
  if (host_) (void)hipHostFree(host_);
  if (dev_) (void)hipFree(dev_);
}

void LaneRounds::round(const std::vector<LaneUnit>* units, Solver* const* solvers, int nLanes, int device, hipStream_t s,
                       int32_t* trialLaunches, int32_t* checkLaunches, int32_t* mixedLaunches) {
  size_t J = 0;
  for (int l = 0; l < nLanes; ++l) J = std::max(J, units[l].size());
  if (J == 0) return;
  if (J > (size_t)kMaxUnits) throw std::runtime_error(who_ + ": more units in a round than argument slots");
  std::vector<SmallTrialsLaunch> tl(J * kBatchLanes);
  std::vector<CheckSmallLaunch> cl(J * kBatchLanes);
  std::vector<char> anyTrials(J, 0);
  char* hostT = static_cast<char*>(host_);
  char* hostC = hostT + J * slotT_;
  for (size_t j = 0; j < J; ++j) {
    for (int l = 0; l < nLanes; ++l) {
      if (j >= units[l].size()) continue;  // (grid 0: the lane takes no part in launch j)
      const LaneUnit& q = units[l][j];
      if (q.hasTrials) { tl[j * kBatchLanes + l] = q.trials; anyTrials[j] = 1; }
      cl[j * kBatchLanes + l] = q.check;
    }
    fillSmallTrialsLanes(&tl[j * kBatchLanes], nLanes, hostT + j * slotT_);
    fillCheckSmallLanes(&cl[j * kBatchLanes], nLanes, hostC + j * slotC_);
  }
  const char* devT = static_cast<const char*>(dev_);
  const char* devC = devT + J * slotT_;
  std::unique_lock<std::mutex> gate = Solver::sharedBeginRound(device, s);
  try {
    PDLP_HIP(hipMemcpyAsync(dev_, host_, J * (slotT_ + slotC_), hipMemcpyHostToDevice, s));
    for (size_t j = 0; j < J; ++j) {
      if (anyTrials[j]) {
        if (launchSmallTrialsLanes(&tl[j * kBatchLanes], nLanes, devT + j * slotT_, s)) ++*mixedLaunches;
        ++*trialLaunches;
      }
      launchCheckSmallLanes(&cl[j * kBatchLanes], nLanes, devC + j * slotC_, s);
      ++*checkLaunches;
    }
  } catch (...) {  // the end of the round is marked on every way out (Solver::BarrierRound)
    try { Solver::sharedEndRound(device, s, gate); } catch (...) {}
    throw;
  }
  Solver::sharedEndRound(device, s, gate);
  for (int l = 0; l < nLanes; ++l)
    if (!units[l].empty()) solvers[l]->laneDownload(s);
  PDLP_HIP(hipStreamSynchronize(s));
  PDLP_HIP(hipGetLastError());  // a launch that failed (bad grid, LDS request, ...) surfaces here
}

namespace {

// One problem's solver, created with the caller's options (its log lines prefixed), destroyed with the lane.
class SolverPoolLane : public PoolLane {
 public:
  SolverPoolLane(const pdlp_problem_t& P, const pdlp_params_t& opt, int32_t k) {
    pdlp_params_t o = opt;
    if (o.log_level >= 1) {
      tap_.sink = opt.log_callback;
      tap_.sinkCtx = opt.log_ctx;
      tap_.prefix = "[problem " + std::to_string(k) + "] ";
      o.log_callback = &LogTap::write;
      o.log_ctx = &tap_;
    }
    s_.reset(new Solver(P, o, 0, 1, nullptr));
  }
  std::string sequentialReason() override {
    // (the shared launches of a pool carry the LP bodies only: pdlp_small.hip k_trials_small_lanes / _mixed)
    if (s_->hasOffDiagonalHessian()) return "off-diagonal Hessian: not in shared pool launches";
    return s_->laneSequentialReason();
  }
  void runAlone(pdlp_result_t* R) override { s_->run(R); }
  void begin() override { s_->laneBegin(); }
  bool idle() override { return s_->laneIdle(); }
  void queue(int32_t ahead, std::vector<LaneUnit>& units) override { s_->laneQueue(ahead, units); }
  LaneVerdict afterRound() override { return s_->laneAfterRound(); }
  void finish(pdlp_result_t* R) override { s_->laneFinish(R); }
  int32_t xcc() override { return s_->laneXcc(); }
  Solver* solver() { return s_.get(); }

 private:
  LogTap tap_;  // (outlives the solver: declared first)
  std::unique_ptr<Solver> s_;
};

// The device behind the driver: the pool's own stream and argument slots; the device gate is taken per round.
class DevicePoolBackend : public PoolBackend {
 public:
  DevicePoolBackend(const pdlp_problem_t* const* P, const pdlp_params_t& opt) : P_(P), opt_(opt), rounds_("pdlp_mi355x_solve_many") {
    PDLP_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
  }
  ~DevicePoolBackend() override {
    if (stream_) {
      (void)hipStreamSynchronize(stream_);
      (void)hipStreamDestroy(stream_);
    }
  }
  std::unique_ptr<PoolLane> create(int32_t k) override { return std::unique_ptr<PoolLane>(new SolverPoolLane(*P_[k], opt_, k)); }
  void round(const std::vector<LaneUnit>* units, PoolLane* const* lanes, int nLanes, int32_t* trialLaunches, int32_t* checkLaunches,
             int32_t* mixedLaunches) override {
    Solver* solvers[kBatchLanes] = {};
    for (int l = 0; l < nLanes && l < kBatchLanes; ++l)
      if (lanes[l]) solvers[l] = static_cast<SolverPoolLane*>(lanes[l])->solver();
    rounds_.round(units, solvers, nLanes, opt_.device, stream_, trialLaunches, checkLaunches, mixedLaunches);
  }

 private:
  const pdlp_problem_t* const* P_;
  pdlp_params_t opt_;
  LaneRounds rounds_;
  hipStream_t stream_ = nullptr;
};

}  // namespace

std::string poolRefusal(int32_t K, const pdlp_problem_t* const* P, const pdlp_params_t* opt, int32_t lanes, const pdlp_result_t* R) {
  const std::string who = "pdlp_mi355x_solve_many: ";
  if (!P || !opt || !R) return who + "null argument";
  if (K < 1) return who + "K = " + std::to_string(K) + " problems (at least 1)";
  if (lanes < 1 || lanes > kBatchLanes) return who + "lanes = " + std::to_string(lanes) + " is outside 1..8 (one lane per XCD)";
  if (opt->algorithm != 0 && opt->algorithm != 1) return "unknown algorithm (0 = cuPDLP-C path, 1 = HiPDLP path)";
  if (const char* why = sessionOneShotReason(*opt)) return who + why;
  for (int32_t k = 0; k < K; ++k) {
    const std::string at = "problem " + std::to_string(k) + ": ";
    if (!P[k]) return at + "null problem";
    if (P[k]->num_nz > (int64_t)INT32_MAX)
      return at + "pdlp_mi355x: the device path indexes the formulated matrix with 32-bit offsets, at most INT32_MAX = 2147483647 nonzeros; "
                  "this problem has " + std::to_string(P[k]->num_nz) + " nonzeros";
    try {
      validateProblem(*P[k]);
    } catch (const std::exception& e) {
      return at + e.what();
    }
  }
  return std::string();
}

void solveMany(int32_t K, const pdlp_problem_t* const* P, const pdlp_params_t* optIn, int32_t lanes, pdlp_result_t* R, int32_t* path,
               pdlp_pool_info_t* info) {
  const std::string refused = poolRefusal(K, P, optIn, lanes, R);  // all before any device call; R and path untouched
  if (!refused.empty()) throw std::runtime_error(refused);
  const pdlp_params_t& opt = *optIn;
  PDLP_HIP(hipSetDevice(opt.device));
  std::vector<int32_t> ownPath;
  if (!path) {
    ownPath.assign((size_t)K, 0);
    path = ownPath.data();
  }
  DevicePoolBackend backend(P, opt);
  PoolDriver driver(lanes, &backend);
  try {
    driver.run(K, R, path);
  } catch (...) {
    if (info) *info = driver.info();
    throw;
  }
  if (info) *info = driver.info();
}

}  // namespace pdlp
