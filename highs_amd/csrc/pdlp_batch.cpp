// pdlp_batch.cpp — the driver of a batch (pdlp_batch.hpp): which variant runs on which lane, the rounds of shared
// launches, the refills and the failure rule.  No device call is made here: lanes and device are the two interfaces.
#include "pdlp_batch.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <stdexcept>

namespace pdlp {

BatchDriver::BatchDriver(std::vector<BatchLane*> lanes, BatchBackend* backend) : lanes_(std::move(lanes)), backend_(backend) {
  memset(&info_, 0, sizeof(info_));
  info_.lanes = (int32_t)lanes_.size();
  for (int l = 0; l < kBatchLanes; ++l) info_.xcc_of_lane[l] = -1;
  snprintf(info_.reason, sizeof(info_.reason), "nothing solved yet");
}

// pdlp_update_t.reserved: the variant's own iteration limit
static int32_t iterLimitOf(const pdlp_update_t& u) { return u.reserved > 0 ? u.reserved : 0; }

void BatchDriver::run(int32_t K, const pdlp_update_t* u, pdlp_result_t* R) {
  if (K < 1) throw std::runtime_error("pdlp_mi355x_batch_run: K = " + std::to_string(K) + " variants (at least 1)");
  if (!u || !R) throw std::runtime_error("pdlp_mi355x_batch_run: null argument");
  // all-or-nothing: every variant is validated before the first one changes a lane
  for (int32_t k = 0; k < K; ++k) {
    try {
      lanes_[0]->validate(u[k]);
    } catch (const std::exception& e) {
      throw std::runtime_error("variant " + std::to_string(k) + ": " + e.what());
    }
  }
  const auto t0 = std::chrono::steady_clock::now();
  const int32_t nLanes = (int32_t)lanes_.size();
  info_.lanes = nLanes;
  info_.lanes_concurrent = 1;
  info_.variants = K;
  info_.trial_launches = info_.check_launches = info_.fallback_variants = 0;
  for (int l = 0; l < kBatchLanes; ++l) info_.xcc_of_lane[l] = -1;
  const std::string why = lanes_[0]->sequentialReason();
  if (!why.empty()) {
    snprintf(info_.reason, sizeof(info_.reason), "sequential: %s", why.c_str());
    runSequential(0, K, u, R);
  } else if (nLanes == 1 || K == 1) {
    snprintf(info_.reason, sizeof(info_.reason), "sequential: %s", nLanes == 1 ? "one lane" : "one variant");
    runSequential(0, K, u, R);
  } else {
    runConcurrent(K, u, R);
  }
  info_.wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

void BatchDriver::runSequential(int32_t first, int32_t K, const pdlp_update_t* u, pdlp_result_t* R) {
  for (int32_t k = first; k < K; ++k) {
    lanes_[0]->setVariant(k, iterLimitOf(u[k]));
    lanes_[0]->update(u[k]);
    lanes_[0]->runAlone(&R[k]);
  }
}

void BatchDriver::runConcurrent(int32_t K, const pdlp_update_t* u, pdlp_result_t* R) {
  const int32_t nLanes = (int32_t)lanes_.size();
  std::vector<int32_t> variantOf((size_t)nLanes, -1);  // the variant a lane is solving, -1: none
  std::vector<char> out((size_t)nLanes, 0);            // the lane has left the concurrent set (the failure rule)
  std::vector<char> ran((size_t)nLanes, 0);            // the lane has taken part in a shared launch of this call
  std::vector<std::pair<int32_t, int32_t>> alone;      // (lane, variant) to be re-solved alone once the others have finished
  std::vector<std::vector<LaneUnit>> units((size_t)nLanes);
  int32_t next = 0, ahead = 1, aheadMax = 16, most = 0;
  for (;;) {
    // refill: a free lane takes the next unsolved variant, the others carry on
    int32_t active = 0;
    for (int32_t l = 0; l < nLanes; ++l) {
      while (variantOf[l] < 0 && !out[l] && next < K) {
        const int32_t k = next++;
        lanes_[l]->setVariant(k, iterLimitOf(u[k]));
        lanes_[l]->update(u[k]);
        lanes_[l]->begin();
        if (lanes_[l]->idle()) lanes_[l]->finish(&R[k]);  // (the iteration limit is reached before the first round)
        else { variantOf[l] = k; ran[l] = 1; }
      }
      if (variantOf[l] >= 0) ++active;
    }
    if (active == 0) break;
    most = std::max(most, active);
    size_t deepest = 0;
    for (int32_t l = 0; l < nLanes; ++l) {
      units[l].clear();
      if (variantOf[l] >= 0) lanes_[l]->queue(ahead, units[l]);
      deepest = std::max(deepest, units[l].size());
    }
    const auto roundBeg = std::chrono::steady_clock::now();
    int32_t nt = 0, nc = 0;
    backend_->round(units.data(), nLanes, &nt, &nc);
    info_.trial_launches += nt;
    info_.check_launches += nc;
    for (int32_t l = 0; l < nLanes; ++l) {
      if (variantOf[l] < 0) continue;
      const LaneVerdict v = lanes_[l]->afterRound();
      if (v == kLaneGoOn) continue;
      if (v == kLaneOver) {
        lanes_[l]->finish(&R[variantOf[l]]);
      } else {
        // the failure rule: the shared launch has changed nothing for this lane (placement, roll call) or the lane is
        // stopped (barrier timeout).  The lane leaves the concurrent set for good — no shared launch is tried again for
        // it — and its variant waits for the ordinary run below.
        alone.emplace_back(l, variantOf[l]);
        out[l] = 1;
      }
      variantOf[l] = -1;
    }
    // queue depth, as one solver chooses it (pdlp_round.hpp), by the deepest lane's units
    const double roundMs = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - roundBeg).count();
    ahead = nextQueueDepth(ahead, aheadMax, (int32_t)deepest, roundMs, false);
  }
  info_.lanes_concurrent = std::max(most, 1);
  for (int32_t l = 0; l < nLanes; ++l)
    if (ran[l] && !out[l]) info_.xcc_of_lane[l] = lanes_[l]->xcc();
  snprintf(info_.reason, sizeof(info_.reason), "concurrent: %d lanes, %d workgroups each", nLanes, lanes_[0]->workBlocks());
  for (const auto& lk : alone) {
    lanes_[lk.first]->runAlone(&R[lk.second]);  // (the lane holds the variant's data: its update went through)
    ++info_.fallback_variants;
  }
  // every lane has failed with variants left: those run one after the other on a lane's own solver
  if (next < K) {
    for (int32_t k = next; k < K; ++k) {
      lanes_[0]->setVariant(k, iterLimitOf(u[k]));
      lanes_[0]->update(u[k]);
      lanes_[0]->runAlone(&R[k]);
      ++info_.fallback_variants;
    }
  }
}

}  // namespace pdlp
