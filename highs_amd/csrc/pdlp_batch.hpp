// pdlp_batch.hpp — up to eight variants of one small LP solved at once, one per XCD (pdlp_mi355x_batch_*).
//
// A batch owns `lanes` ordinary solvers of ONE problem.  Where a solver's trial loop runs XCD-local (at most 32 work
// blocks: seven of the eight XCDs idle by construction) the lanes' loops share launches: k_trials_small_lanes /
// k_check_small_lanes give workgroup b to lane b & 7, every lane running — on its own state, barrier words and vectors —
// exactly what its solo launch runs.  Nothing is synchronised between lanes: step sizes, restarts, check schedule and
// halt are each lane's own, so the bits of every result are those of a solo update + run.  A lane whose variant has ended
// takes the next one while the others carry on.  Everywhere else batch_run is a loop of update + run on lane 0.
//
// A variant (pdlp_variant_t) is new data and, through pdlp_mi355x_batch_run_values, new matrix and Hessian VALUES on P's
// patterns; pdlp_mi355x_batch_run wraps each of its updates into a variant without values.  Value updates keep row order,
// task plans, chunk sizes, the XCD map and the persistent loop, so whether the launches are shared depends on the pattern
// and the options alone.
//
// The driver (BatchDriver) sees its lanes and the device only through the two interfaces below, so that it also runs
// against canned lanes on a machine without a device.
#pragma once
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "pdlp_kernels.hpp"
#include "pdlp_host.hpp"
#include "pdlp_round.hpp"

namespace pdlp {

class Solver;

// One unit of a lane's queue: [trial batch to the next scheduled check][check] of the round's plan (pdlp_round.hpp), as
// launch records.
struct LaneUnit {
  bool hasTrials = false;  // false: the entry's check alone
  SmallTrialsLaunch trials;
  CheckSmallLaunch check;
};

enum LaneVerdict : int { kLaneGoOn = 0, kLaneOver = 1, kLaneFailed = 2 };

using Variant = pdlp_variant_t;
// new values, or a count that claims some (refused as pdlp_mi355x_update_values refuses it): not a plain pdlp_mi355x_update
inline bool hasValues(const Variant& v) { return v.a_value || v.q_value || v.num_nz != 0 || v.num_q_nz != 0; }
constexpr const char* kEntryBatchRun = "pdlp_mi355x_batch_run";
constexpr const char* kEntryBatchRunValues = "pdlp_mi355x_batch_run_values";
constexpr const char* kEntryBatchRunDevice = "pdlp_mi355x_batch_run_device";

// Where the arrays of ONE call live: in host memory (batch_run, batch_run_values) or in HBM on the batch's device
// (batch_run_device, pdlp_batch_resident.hpp).  A call never mixes the two: what a lane restores comes from the copy of P
// that lives where the variants do.
enum LaneMode : int { kLaneHost = 0, kLaneDevice = 1 };

// What of P an update can change, as pointers and counts: a BaseData's vectors, or their copy in HBM (the plan hands the
// pointers on and never reads through them).
struct BaseView {
  const double *cost = nullptr, *colLower = nullptr, *colUpper = nullptr, *rowLower = nullptr, *rowUpper = nullptr;
  const double *aValue = nullptr, *qValue = nullptr;
  int64_t nnz = 0, qSlots = 0;
  double offset = 0.0;
};
// ... kept on the host: variant k is P with v[k] applied, whatever variant the lane solved before — so what an earlier
// variant changed on a lane and this one leaves alone goes back to P's values.
struct BaseData {
  std::vector<double> cost, colLower, colUpper, rowLower, rowUpper, aValue, qValue;
  double offset = 0.0;
  explicit BaseData(const pdlp_problem_t& P);
  BaseView view() const;
};

// The ONE update call that takes a lane's solver, which differs from P in the arrays `differs` names, to variant v: what v
// gives, P's array for what it leaves alone but the solver differs in, nothing (NULL: unchanged) for the rest.
enum : int { kLaneCost = 1, kLaneColLower = 2, kLaneColUpper = 4, kLaneRows = 8, kLaneOffset = 16, kLaneMatrix = 32, kLaneHessian = 64 };
enum LaneCall : int { kCallUpdate = 0, kCallUpdateMatrix = 1, kCallUpdateValues = 2 };
struct LaneUpdatePlan {
  Variant v;      // the arguments of the call
  int now = 0;    // the arrays in which the solver differs from P afterwards
  LaneCall call = kCallUpdate;  // no value array: the plain update; a_value alone: update_matrix (which is update_values on a
                                // Hessian-updatable solver); else update_values
};
LaneUpdatePlan planLaneUpdate(const Variant& v, int differs, const BaseView& base);

// What the driver asks of a resident solver (SolverLane: Solver's lane steps, pdlp_solver.hpp).
class BatchLane {
 public:
  virtual ~BatchLane() = default;
  virtual std::string sequentialReason() = 0;  // empty: the launches can be shared
  virtual int32_t workBlocks() = 0;
  // kLaneDevice: what follows in this call — update, finish, runAlone — takes the variants' arrays and writes the results'
  // vectors in HBM, and restores from P's copy there.  Set on every lane at the start of every call.
  virtual void setMode(LaneMode mode) = 0;
  virtual void validate(const Variant& v) = 0;  // throws with the words of the update entry v maps to; changes nothing
  // kLaneDevice, asked of lane 0 once per call: all K variants and results at once, in the order of pdlp_batch_resident.hpp
  // (value-free refusals, the pointer check, one validation launch); throws "variant k: ..." / "result k: ..."; changes nothing
  virtual void validateDevice(int32_t K, const Variant* v, const pdlp_result_t* R) = 0;
  virtual void setVariant(int32_t k, int32_t iterLimit) = 0;  // log prefix and iteration limit (0: the batch's) of what follows
  virtual void update(const Variant& v) = 0;
  virtual void runAlone(pdlp_result_t* R) = 0;  // the ordinary run, with its own fall-backs
  virtual void begin() = 0;
  virtual bool idle() = 0;
  virtual void queue(int32_t ahead, std::vector<LaneUnit>& units) = 0;
  virtual LaneVerdict afterRound() = 0;
  virtual void finish(pdlp_result_t* R) = 0;
  virtual int32_t xcc() = 0;
};

// One round on the device: launch j = the j-th units of all lanes that have one, [trials] then [check] in one launch each
// behind ONE take of the device gate; every taking lane's state record downloaded behind them; one synchronisation.
class BatchBackend {
 public:
  virtual ~BatchBackend() = default;
  virtual void round(const std::vector<LaneUnit>* units, int nLanes, int32_t* trialLaunches, int32_t* checkLaunches) = 0;
};

class BatchDriver {
 public:
  BatchDriver(std::vector<BatchLane*> lanes, BatchBackend* backend);
  // entry: named in the refusals; mode: where the arrays of v and R live
  void run(int32_t K, const Variant* v, pdlp_result_t* R, const char* entry = kEntryBatchRun, LaneMode mode = kLaneHost);
  const pdlp_batch_info_t& info() const { return info_; }

 private:
  void runSequential(int32_t first, int32_t K, const Variant* v, pdlp_result_t* R);
  void runConcurrent(int32_t K, const Variant* v, pdlp_result_t* R);
  std::vector<BatchLane*> lanes_;
  BatchBackend* backend_;
  pdlp_batch_info_t info_{};
};

// Refusals of pdlp_mi355x_batch_create that need no device: nullptr, or the message.
std::string batchCreateRefusal(const pdlp_params_t& opt, int32_t lanes);
// K < 1 and null arrays, as both run entries refuse them.  Throws.
void refuseBatchArguments(const char* entry, int32_t K, const void* variants, const void* results);
// Refusals of one variant of pdlp_mi355x_batch_run_values that look at no matrix or Hessian VALUE, for a batch created on P
// with opt (the batch's own DATA bit is added here): empty, or the words of the update entry the variant maps to.
std::string batchVariantRefusal(const pdlp_problem_t& P, const pdlp_params_t& opt, const Variant& v);
// ... of pdlp_mi355x_batch_run_device: the same, from the pointers' being NULL or not alone (no array is read: the row
// kinds are compared on the device)
std::string batchVariantDeviceRefusal(const pdlp_problem_t& P, const pdlp_params_t& opt, const Variant& v);

// The batch behind the C ABI: the solvers, their lanes, the device backend and the driver.
class Batch {
 public:
  Batch(const pdlp_problem_t& P, const pdlp_params_t& opt, int32_t lanes);
  ~Batch();
  void run(int32_t K, const pdlp_update_t* u, pdlp_result_t* R);
  void runValues(int32_t K, const Variant* v, pdlp_result_t* R);
  // pdlp_mi355x_batch_run_device: every array of v[k] and every vector of R[k] in HBM on the batch's device
  void runDevice(int32_t K, const Variant* vDev, pdlp_result_t* RDev, hipStream_t callerStream);
  // Test hook: the validation launch alone on vDev (after the pointer check), with nRec >= K records initialised; all nRec
  // records, three int32 each, into out
  void variantRecords(int32_t K, const Variant* vDev, int32_t nRec, int32_t* out);
  const pdlp_batch_info_t& info() const { return driver_->info(); }

 private:
  struct Impl;
  std::unique_ptr<Impl> impl_;
  std::unique_ptr<BatchDriver> driver_;
};

}  // namespace pdlp
