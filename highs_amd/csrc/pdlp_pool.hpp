// pdlp_pool.hpp — up to eight DIFFERENT small LPs solved at once, one per XCD (pdlp_mi355x_solve_many).
//
// A pool is one call: K problems, `lanes` lanes.  A free lane takes the next problem in the caller's order, creates its
// ordinary solver and — where that solver's trial loop runs XCD-local — joins the shared launches of pdlp_batch.hpp
// (k_trials_small_lanes / k_check_small_lanes: workgroup b works for lane b & 7), now with a grid and a number of barriers
// per trial of its own.  Nothing is synchronised between lanes, so the bits of every result are those of a solo
// create + run + destroy.  A problem whose solver does not qualify is solved right there by the ordinary run.
//
// The driver (PoolDriver) sees its solvers and the device only through the two interfaces below, so that it also runs
// against canned lanes on a machine without a device (tools/pool_driver_check.cpp).
#pragma once
#include <cstdint>
#include <cstdio>
#include <memory>
#include <string>
#include <vector>

#include "pdlp_batch.hpp"

namespace pdlp {

// Log lines of a lane: `prefix` ("[variant k] ", "[problem k] ") in front of every line, then the caller's sink (NULL: stdout).
struct LogTap {
  void (*sink)(void*, int, const char*) = nullptr;
  void* sinkCtx = nullptr;
  std::string prefix;
  bool lineStart = true;
  static void write(void* ctx, int level, const char* text) {
    LogTap& t = *static_cast<LogTap*>(ctx);
    std::string out;
    for (const char* p = text; *p; ++p) {
      if (t.lineStart && *p != '\n') out += t.prefix;
      t.lineStart = *p == '\n';
      out += *p;
    }
    if (t.sink) t.sink(t.sinkCtx, level, out.c_str());
    else { fputs(out.c_str(), stdout); fflush(stdout); }
  }
};

// The argument slots of a round and the round itself (BatchBackend::round's words), on a stream and behind a device gate
// that are the caller's: a batch gives its lane 0's, a pool its own — pool solvers come and go.
class LaneRounds {
 public:
  explicit LaneRounds(const char* who);  // `who` opens the messages ("pdlp_mi355x_batch_run")
  ~LaneRounds();
  LaneRounds(const LaneRounds&) = delete;
  LaneRounds& operator=(const LaneRounds&) = delete;
  // solvers[l] downloads its state record behind the launches if units[l] is not empty; *mixedLaunches counts the trial
  // launches that carried lanes of two and of three barriers per trial together
  void round(const std::vector<LaneUnit>* units, Solver* const* solvers, int nLanes, int device, hipStream_t s,
             int32_t* trialLaunches, int32_t* checkLaunches, int32_t* mixedLaunches);

 private:
  static constexpr int kMaxUnits = 20;  // a round queues the entry's check and at most 16 units per lane
  std::string who_;
  size_t slotT_ = 0, slotC_ = 0;
  void* host_ = nullptr;
  void* dev_ = nullptr;
};

// What the driver asks of one problem's solver (Solver's lane steps, pdlp_solver.hpp).  Destroying it frees the solver.
class PoolLane {
 public:
  virtual ~PoolLane() = default;
  virtual std::string sequentialReason() = 0;    // empty: the launches can be shared
  virtual void runAlone(pdlp_result_t* R) = 0;   // the ordinary run, with its own fall-backs
  virtual void begin() = 0;
  virtual bool idle() = 0;
  virtual void queue(int32_t ahead, std::vector<LaneUnit>& units) = 0;
  virtual LaneVerdict afterRound() = 0;
  virtual void finish(pdlp_result_t* R) = 0;
  virtual int32_t xcc() = 0;
};

// The device as the driver sees it: create problem k's solver (opt as given), and one round (BatchBackend::round) for the
// solvers that sit in the lanes — lanes[l] == nullptr: lane l is empty.
class PoolBackend {
 public:
  virtual ~PoolBackend() = default;
  virtual std::unique_ptr<PoolLane> create(int32_t k) = 0;
  virtual void round(const std::vector<LaneUnit>* units, PoolLane* const* lanes, int nLanes, int32_t* trialLaunches,
                     int32_t* checkLaunches, int32_t* mixedLaunches) = 0;
};

class PoolDriver {
 public:
  PoolDriver(int32_t lanes, PoolBackend* backend);
  // path[k] (never null here) = PDLP_POOL_* of problem k, 0 while it is not solved.  Throws "problem k: ..." where a
  // create or a solve throws; every solver is destroyed by then, and what was finished stays in R and path.
  void run(int32_t K, pdlp_result_t* R, int32_t* path);
  const pdlp_pool_info_t& info() const { return info_; }

 private:
  void runOneByOne(int32_t first, int32_t K, pdlp_result_t* R, int32_t* path, int32_t as);
  void runConcurrent(int32_t K, pdlp_result_t* R, int32_t* path);
  std::unique_ptr<PoolLane> createFor(int32_t k);
  void noteAlone(const std::string& why);
  int32_t nLanes_;
  PoolBackend* backend_;
  pdlp_pool_info_t info_{};
};

// Refusals of pdlp_mi355x_solve_many that need no device: empty, or the message.
std::string poolRefusal(int32_t K, const pdlp_problem_t* const* P, const pdlp_params_t* opt, int32_t lanes, const pdlp_result_t* R);

// The call behind the C ABI: the refusals, the device backend, the driver.  Throws with the library's words.
void solveMany(int32_t K, const pdlp_problem_t* const* P, const pdlp_params_t* opt, int32_t lanes, pdlp_result_t* R,
               int32_t* path, pdlp_pool_info_t* info);

}  // namespace pdlp
