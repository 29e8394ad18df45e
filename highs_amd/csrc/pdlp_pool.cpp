// pdlp_pool.cpp — the driver of a pool (pdlp_pool.hpp): which problem runs on which lane, the creates, the rounds of shared
// launches, the refills, the problems that run alone and the failure rule.  No device call is made here: solvers and device
// are the two interfaces.
#include "pdlp_pool.hpp"

#include <algorithm>
#include <chrono>
#include <cstring>
#include <stdexcept>

namespace pdlp {

namespace {
double since(std::chrono::steady_clock::time_point t0) {
  return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}
[[noreturn]] void rethrowFor(int32_t k, const std::exception& e) {
  throw std::runtime_error("problem " + std::to_string(k) + ": " + e.what());
}
}  // namespace

PoolDriver::PoolDriver(int32_t lanes, PoolBackend* backend) : nLanes_(lanes), backend_(backend) {
  memset(&info_, 0, sizeof(info_));
  info_.lanes = lanes;
  for (int l = 0; l < kBatchLanes; ++l) info_.xcc_of_lane[l] = -1;
  snprintf(info_.reason, sizeof(info_.reason), "nothing solved yet");
}

std::unique_ptr<PoolLane> PoolDriver::createFor(int32_t k) {
  const auto t0 = std::chrono::steady_clock::now();
  try {
    std::unique_ptr<PoolLane> p = backend_->create(k);
    info_.create_seconds += since(t0);
    return p;
  } catch (const std::exception& e) {
    rethrowFor(k, e);
  }
}

// the reason of the FIRST problem that did not qualify
void PoolDriver::noteAlone(const std::string& why) {
  if (info_.alone_problems++ == 0) snprintf(info_.reason, sizeof(info_.reason), "%s", why.c_str());
}

void PoolDriver::run(int32_t K, pdlp_result_t* R, int32_t* path) {
  const auto t0 = std::chrono::steady_clock::now();
  memset(&info_, 0, sizeof(info_));
  info_.problems = K;
  info_.lanes = nLanes_;
  info_.lanes_concurrent = 1;
  for (int l = 0; l < kBatchLanes; ++l) info_.xcc_of_lane[l] = -1;
  for (int32_t k = 0; k < K; ++k) path[k] = PDLP_POOL_NOT_RUN;
  try {
    if (nLanes_ == 1 || K == 1) {
      snprintf(info_.reason, sizeof(info_.reason), "sequential: %s", nLanes_ == 1 ? "one lane" : "one problem");
      runOneByOne(0, K, R, path, PDLP_POOL_ALONE);
    } else {
      runConcurrent(K, R, path);
    }
  } catch (...) {
    info_.wall_seconds = since(t0);
    throw;
  }
  info_.wall_seconds = since(t0);
}

// a loop of ordinary solves: create, run, destroy
void PoolDriver::runOneByOne(int32_t first, int32_t K, pdlp_result_t* R, int32_t* path, int32_t as) {
  for (int32_t k = first; k < K; ++k) {
    std::unique_ptr<PoolLane> p = createFor(k);
    try {
      p->runAlone(&R[k]);
    } catch (const std::exception& e) {
      rethrowFor(k, e);
    }
    path[k] = as;
    ++(as == PDLP_POOL_ALONE ? info_.alone_problems : info_.fallback_problems);
  }
}

void PoolDriver::runConcurrent(int32_t K, pdlp_result_t* R, int32_t* path) {
  const int32_t nLanes = nLanes_;
  // At most `nLanes` solvers (and the one being created) exist at a time: lane[l] holds the solver of the problem lane l is
  // solving — or, once the lane has left the shared launches (out[l]), of the problem that waits for its run alone.
  std::vector<std::unique_ptr<PoolLane>> lane((size_t)nLanes);
  std::vector<PoolLane*> taking((size_t)nLanes, nullptr);  // the solvers inside the shared launches
  std::vector<int32_t> problemOf((size_t)nLanes, -1);
  std::vector<char> out((size_t)nLanes, 0);
  std::vector<std::vector<LaneUnit>> units((size_t)nLanes);
  int32_t next = 0, ahead = 1, aheadMax = 16, most = 0;
  snprintf(info_.reason, sizeof(info_.reason), "concurrent: %d lanes", nLanes);
  for (;;) {
    // refill: a free lane takes the next unsolved problem in the caller's order, the others carry on
    int32_t active = 0;
    for (int32_t l = 0; l < nLanes; ++l) {
      while (!taking[l] && !out[l] && next < K) {
        const int32_t k = next++;
        std::unique_ptr<PoolLane> p = createFor(k);
        try {
          const std::string why = p->sequentialReason();
          if (!why.empty()) {  // does not qualify: solved right here by the ordinary run, the lane takes the next problem
            noteAlone(why);
            p->runAlone(&R[k]);
            path[k] = PDLP_POOL_ALONE;
            continue;
          }
          p->begin();
          if (p->idle()) {  // (the iteration limit is reached before the first round)
            p->finish(&R[k]);
            path[k] = PDLP_POOL_SHARED;
            ++info_.shared_problems;
            continue;
          }
        } catch (const std::exception& e) {
          rethrowFor(k, e);
        }
        lane[l] = std::move(p);
        taking[l] = lane[l].get();
        problemOf[l] = k;
      }
      if (taking[l]) ++active;
    }
    if (active == 0) break;
    most = std::max(most, active);
    size_t deepest = 0;
    for (int32_t l = 0; l < nLanes; ++l) {
      units[l].clear();
      if (taking[l]) {
        try {
          taking[l]->queue(ahead, units[l]);
        } catch (const std::exception& e) {
          rethrowFor(problemOf[l], e);
        }
      }
      deepest = std::max(deepest, units[l].size());
    }
    const auto roundBeg = std::chrono::steady_clock::now();
    int32_t nt = 0, nc = 0, nm = 0;
    backend_->round(units.data(), taking.data(), nLanes, &nt, &nc, &nm);
    info_.trial_launches += nt;
    info_.check_launches += nc;
    info_.mixed_launches += nm;
    for (int32_t l = 0; l < nLanes; ++l) {
      if (!taking[l]) continue;
      const int32_t k = problemOf[l];
      try {
        const LaneVerdict v = taking[l]->afterRound();
        if (v == kLaneGoOn) continue;
        if (v == kLaneOver) {
          taking[l]->finish(&R[k]);
          info_.xcc_of_lane[l] = taking[l]->xcc();
          path[k] = PDLP_POOL_SHARED;
          ++info_.shared_problems;
          lane[l].reset();  // the finished problem's solver goes before the lane refills
          problemOf[l] = -1;
        } else {
          // the failure rule: the shared launch has changed nothing for this lane (placement, roll call) or the lane is
          // stopped (barrier timeout).  The lane leaves the concurrent set for good — no shared launch is tried again for
          // it — and its problem waits, in its solver, for the ordinary run below.
          out[l] = 1;
          info_.xcc_of_lane[l] = -1;
        }
      } catch (const std::exception& e) {
        rethrowFor(k, e);
      }
      taking[l] = nullptr;
    }
    // queue depth, as one solver chooses it (pdlp_round.hpp), by the deepest lane's units
    ahead = nextQueueDepth(ahead, aheadMax, (int32_t)deepest, since(roundBeg) * 1e3, false);
  }
  info_.lanes_concurrent = std::max(most, 1);
  for (int32_t l = 0; l < nLanes; ++l) {
    if (!out[l]) continue;
    const int32_t k = problemOf[l];
    try {
      lane[l]->runAlone(&R[k]);
    } catch (const std::exception& e) {
      rethrowFor(k, e);
    }
    path[k] = PDLP_POOL_FALLBACK;
    ++info_.fallback_problems;
    lane[l].reset();
  }
  // every lane has failed with problems left: those run one after the other
  if (next < K) runOneByOne(next, K, R, path, PDLP_POOL_FALLBACK);
}

}  // namespace pdlp
