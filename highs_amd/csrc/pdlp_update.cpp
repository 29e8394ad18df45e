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
}  // namespace

void checkUpdateShape(const pdlp_update_t& u) {
  if ((u.row_lower != nullptr) != (u.row_upper != nullptr))
    throw std::runtime_error(std::string("pdlp_mi355x_update: row_lower and row_upper are given together or not at all (") +
                             (u.row_lower ? "row_upper" : "row_lower") + " is NULL)");
  const int given = (u.start_col_value ? 1 : 0) + (u.start_row_value ? 1 : 0) + (u.start_row_dual ? 1 : 0);
  if (given != 0 && given != 3)
    throw std::runtime_error("pdlp_mi355x_update: partial start: start_col_value, start_row_value and start_row_dual are given "
                             "all three (hot start) or none (cold start), " + std::to_string(given) + " of 3 are given");
}

int32_t firstKindChange(const int32_t* rowKind, int32_t m, const double* rowLower, const double* rowUpper) {
  for (int32_t i = 0; i < m; ++i)
    if (rowKindOf(rowLower[i], rowUpper[i]) != rowKind[i]) return i;
  return m;
}

void throwKindChange(int32_t row, int32_t was, int32_t now) {
  throw std::runtime_error("pdlp_mi355x_update: row " + std::to_string(row) + " would change its kind from " + kindName(was) +
                           " to " + kindName(now) + " (the kind decides row order, slack columns and signs: create a new solver)");
}

void hostReplayUpdate(const pdlp_update_t& u, StandardForm& F) {
  checkUpdateShape(u);
  if (!F.keepPasses) throw std::runtime_error("pdlp_mi355x_update: the form did not keep its scaling passes");
  const int32_t n0 = F.n0, n = F.n, m = F.m;
  const int32_t mask = updateMask(u);
  if (mask & kUpdRows) {
    const int32_t bad = firstKindChange(F.rowKind.data(), m, u.row_lower, u.row_upper);
    if (bad < m) throwKindChange(bad, F.rowKind[bad], rowKindOf(u.row_lower[bad], u.row_upper[bad]));
  }
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
      for (int32_t p = 0; p < F.nPass; ++p) r /= F.rsPass[(size_t)p * m + ni];
      F.rhs[ni] = r;
    }
  if (mask & kUpdCost) F.normCost = unscaledNormCost(u.col_cost, n0, F.sense);
  if (mask & kUpdRows) F.normRhs = unscaledNormRhs(u.row_lower, u.row_upper, F.rowKind.data(), m);
  if (u.has_offset) F.offset = u.offset;
}

void SolverBase::update(const pdlp_update_t&) {
  throw std::runtime_error("pdlp_mi355x_update: HiPDLP solvers (algorithm = 1) do not take updates");
}

// The held solver is brought to the state of a fresh create() on the modified problem.  Everything that can be refused
// is refused before the first write to the solver's vectors: the caller's row bounds go to a staging buffer, the
// validation kernel reads only that and the kept kinds.
void Solver::update(const pdlp_update_t& u) {
  using clock = std::chrono::steady_clock;
  const auto t0 = clock::now();
  auto since = [](clock::time_point a) { return std::chrono::duration<double>(clock::now() - a).count(); };
  if (sharded_)
    throw std::runtime_error("pdlp_mi355x_update: sharded solvers (pdlp_mi355x_create_sharded) do not take updates");
  if (!updatable_)
    throw std::runtime_error("pdlp_mi355x_update: the solver was not created for updates (pdlp_params_t.updatable = 0)");
  checkUpdateShape(u);
  const int32_t n0 = F_.n0, n = F_.n, m = F_.m;
  const int32_t mask = updateMask(u);
  PDLP_HIP(hipSetDevice(opt_.device));
  PDLP_HIP(hipStreamSynchronize(stream_));
  if (updIn_.size() == 0) {
    updIn_.alloc((size_t)3 * n0 + (size_t)2 * m);
    updBad_.alloc(1);
  }
  double* dCost = updIn_.get();
  double* dColLo = dCost + n0;
  double* dColUp = dColLo + n0;
  double* dRowLo = dColUp + n0;
  double* dRowUp = dRowLo + m;
  auto put = [&](double* dev, const double* host, int32_t count) {
    if (count > 0) PDLP_HIP(hipMemcpyAsync(dev, host, sizeof(double) * (size_t)count, hipMemcpyHostToDevice, stream_));
  };
  if (mask & kUpdRows) {
    put(dRowLo, u.row_lower, m);
    put(dRowUp, u.row_upper, m);
    int32_t bad = m;
    PDLP_HIP(hipMemcpyAsync(updBad_.get(), &bad, sizeof(int32_t), hipMemcpyHostToDevice, stream_));
    launchUpdateValidate(dRowLo, dRowUp, rowKindDev_.get(), m, updBad_.get(), stream_);
    PDLP_HIP(hipMemcpyAsync(&bad, updBad_.get(), sizeof(int32_t), hipMemcpyDeviceToHost, stream_));
    PDLP_HIP(hipStreamSynchronize(stream_));
    if (bad < m) throwKindChange(bad, F_.rowKind[bad], rowKindOf(u.row_lower[bad], u.row_upper[bad]));
  }
  // ---- nothing below is refused ----
  if (mask & kUpdCost) put(dCost, u.col_cost, n0);
  if (mask & kUpdColLower) put(dColLo, u.col_lower, n0);
  if (mask & kUpdColUpper) put(dColUp, u.col_upper, n0);
  PDLP_HIP(hipStreamSynchronize(stream_));
  updSeconds_[0] = since(t0);

  auto t1 = clock::now();
  launchUpdateCols(mask, dCost, dColLo, dColUp, dRowLo, dRowUp, slackRowDev_.get(), F_.sense, n0, n, csPass_.get(), nPass_,
                   cost_.get(), lower_.get(), upper_.get(), stream_);
  if (mask & kUpdRows)
    launchUpdateRows(dRowLo, dRowUp, rowKindDev_.get(), rowNewIdxDev_.get(), m, rsPass_.get(), nPass_, rhs_.get(), stream_);
  PDLP_HIP(hipStreamSynchronize(stream_));
  updSeconds_[1] = since(t1);

  // termination norms of the unscaled data and the left-to-right sums of the scaled c, b (PDHG_Init_Step_Sizes), by the
  // host loops of the set-up
  t1 = clock::now();
  if (mask & kUpdCost) {
    F_.normCost = unscaledNormCost(u.col_cost, n0, F_.sense);
    std::vector<double> hc((size_t)n);
    cost_.download(hc.data(), (size_t)n, stream_);
    PDLP_HIP(hipStreamSynchronize(stream_));
    sumCost2_ = 0.0;
    for (double v : hc) sumCost2_ += v * v;
  }
  if (mask & kUpdRows) {
    F_.normRhs = unscaledNormRhs(u.row_lower, u.row_upper, F_.rowKind.data(), m);
    std::vector<double> hb((size_t)m);
    rhs_.download(hb.data(), (size_t)m, stream_);
    PDLP_HIP(hipStreamSynchronize(stream_));
    sumRhs2_ = 0.0;
    for (double v : hb) sumRhs2_ += v * v;
  }
  if (u.has_offset) F_.offset = u.offset;
  updSeconds_[2] = since(t1);

  // the fused slab trial's per-block bounds; the captured batch bakes IterVecs::lowerUniform in (the vectors' addresses
  // have not changed), so only a flip of that flag needs a new graph
  t1 = clock::now();
  bool recapture = false;
  if (fused_ && (mask & (kUpdColLower | kUpdColUpper | kUpdRows))) {
    const int32_t before = vecs_.lowerUniform;
    const int32_t after = refreshBlockBounds() ? 1 : 0;
    recapture = before != after;
  }
  updSeconds_[3] = since(t1);

  // start of the next run
  if (u.start_col_value) {
    setHotStart(u.start_col_value, u.start_row_value, u.start_row_dual);
  } else {
    hasStart_ = false;
    startX_.clear();
    startY_.clear();
  }

  t1 = clock::now();
  stPar_ = graphExec_ && !recapture ? graphPar_ : 0;  // the state slot a fresh solver starts from / the kept graph was captured with
  reset();
  stalledRounds_ = 0;
  stalledSince_ = 0;
  updSeconds_[5] = since(t1);
  t1 = clock::now();
  if (recapture && graphExec_) {
    (void)hipGraphExecDestroy(graphExec_);
    graphExec_ = nullptr;
    captureGraph();
  }
  PDLP_HIP(hipStreamSynchronize(stream_));
  updSeconds_[4] = since(t1);
  setupSeconds_ = since(t0);
}

}  // namespace pdlp
