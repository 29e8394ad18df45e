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

BaseData::BaseData(const pdlp_problem_t& P)
    : cost(P.col_cost, P.col_cost + P.num_col), colLower(P.col_lower, P.col_lower + P.num_col),
      colUpper(P.col_upper, P.col_upper + P.num_col), rowLower(P.row_lower, P.row_lower + P.num_row),
      rowUpper(P.row_upper, P.row_upper + P.num_row), offset(P.offset) {
  const int64_t nnz = P.num_col > 0 && P.a_start ? (int64_t)P.a_start[P.num_col] : 0;
  if (nnz > 0 && P.a_value) aValue.assign(P.a_value, P.a_value + nnz);
  const int64_t slots = P.q_dim > 0 && P.q_start && P.q_index && P.q_value ? (int64_t)P.q_start[P.q_dim] : 0;
  if (slots > 0) qValue.assign(P.q_value, P.q_value + slots);
}

BaseView BaseData::view() const {
  BaseView b;
  b.cost = cost.data(); b.colLower = colLower.data(); b.colUpper = colUpper.data();
  b.rowLower = rowLower.data(); b.rowUpper = rowUpper.data();
  b.aValue = aValue.data(); b.qValue = qValue.data();
  b.nnz = (int64_t)aValue.size(); b.qSlots = (int64_t)qValue.size();
  b.offset = offset;
  return b;
}

LaneUpdatePlan planLaneUpdate(const Variant& v, int differs, const BaseView& base) {
  LaneUpdatePlan plan;
  plan.v = v;
  pdlp_update_t& u = plan.v.u;
  int now = 0;
  auto take = [&](const double*& field, const double* kept, int bit) {
    if (field) now |= bit;
    else if (differs & bit) field = kept;
  };
  take(u.col_cost, base.cost, kLaneCost);
  take(u.col_lower, base.colLower, kLaneColLower);
  take(u.col_upper, base.colUpper, kLaneColUpper);
  if (u.row_lower) now |= kLaneRows;  // (given together: validated)
  else if (differs & kLaneRows) { u.row_lower = base.rowLower; u.row_upper = base.rowUpper; }
  if (u.has_offset) now |= kLaneOffset;
  else if (differs & kLaneOffset) { u.has_offset = 1; u.offset = base.offset; }
  take(plan.v.a_value, base.aValue, kLaneMatrix);
  if (!(now & kLaneMatrix) && plan.v.a_value) plan.v.num_nz = base.nnz;
  take(plan.v.q_value, base.qValue, kLaneHessian);
  if (!(now & kLaneHessian) && plan.v.q_value) plan.v.num_q_nz = base.qSlots;
  plan.now = now;
  plan.call = plan.v.q_value ? kCallUpdateValues : plan.v.a_value ? kCallUpdateMatrix : kCallUpdate;
  return plan;
}

void refuseBatchArguments(const char* entry, int32_t K, const void* variants, const void* results) {
  if (K < 1) throw std::runtime_error(std::string(entry) + ": K = " + std::to_string(K) + " variants (at least 1)");
  if (!variants || !results) throw std::runtime_error(std::string(entry) + ": null argument");
}

void BatchDriver::run(int32_t K, const Variant* u, pdlp_result_t* R, const char* entry, LaneMode mode) {
  refuseBatchArguments(entry, K, u, R);
  for (BatchLane* l : lanes_) l->setMode(mode);  // (per call: a refusal below leaves nothing behind)
  // all-or-nothing: every variant is validated before the first one changes a lane
  if (mode == kLaneDevice) {
    lanes_[0]->validateDevice(K, u, R);  // (the arrays cannot be read here: one pass over all of them, on the device)
  } else {
    for (int32_t k = 0; k < K; ++k) {
      try {
        lanes_[0]->validate(u[k]);
      } catch (const std::exception& e) {
        throw std::runtime_error("variant " + std::to_string(k) + ": " + e.what());
      }
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

void BatchDriver::runSequential(int32_t first, int32_t K, const Variant* u, pdlp_result_t* R) {
  for (int32_t k = first; k < K; ++k) {
    lanes_[0]->setVariant(k, iterLimitOf(u[k].u));
    lanes_[0]->update(u[k]);
    lanes_[0]->runAlone(&R[k]);
  }
}

void BatchDriver::runConcurrent(int32_t K, const Variant* u, pdlp_result_t* R) {
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
        lanes_[l]->setVariant(k, iterLimitOf(u[k].u));
        lanes_[l]->update(u[k]);
        // A value update keeps every pattern, so the lane still qualifies; were it ever not to, its variant goes the way
        // of the failure rule below: solved alone afterwards (the lane holds the variant), no shared launch for the lane.
        if (hasValues(u[k]) && !lanes_[l]->sequentialReason().empty()) {
          alone.emplace_back(l, k);
          out[l] = 1;
          break;
        }
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
      lanes_[0]->setVariant(k, iterLimitOf(u[k].u));
      lanes_[0]->update(u[k]);
      lanes_[0]->runAlone(&R[k]);
      ++info_.fallback_variants;
    }
  }
}

}  // namespace pdlp
