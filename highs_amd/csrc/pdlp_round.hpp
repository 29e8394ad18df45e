// pdlp_round.hpp — the schedule of a device-driven round, as pure functions: which iterations carry a
// check, how the stretch to the next one is cut into units [trials][check], and how many units the host queues before it
// looks at the device again.  One solver alone (Solver::doSolveDevice) and a lane of a batch or a pool (Solver::laneQueue)
// walk the same plan; nothing here calls the device or touches a solver, so the plan is also checked on a machine without
// one (tools/round_plan_check.cpp).
#pragma once
#include <algorithm>
#include <climits>
#include <cstdint>

namespace pdlp {

constexpr int32_t kReleaseInterval = 40;  // CUPDLP_RELEASE_INTERVAL, cupdlp_defs.h:39: the check interval unless one is set
constexpr int32_t kRoundMaxTodo = 4 * kReleaseInterval;  // trials of one unit, also where no check falls that soon
constexpr int32_t kRoundMaxUnits = 16;  // trial units of one round (LaneRounds::kMaxUnits keeps argument slots for them)
constexpr int32_t kRoundSpareTrials = 8;  // what a persistent launch may run beyond its todo, for rejected trials

// The first iteration behind `it` at which the reference checks (cupdlp_solver.c:953-962): every iteration below 10, every
// interval-th one, and the last one of the iteration limit.
inline int32_t nextCheckIter(int32_t it, int32_t interval, int32_t iterLimit) {
  int64_t next;
  if (it + 1 < 10) next = it + 1;
  else next = ((int64_t)it / interval + 1) * interval;
  const int64_t last = (int64_t)iterLimit - 1;
  if (last > it && last < next) next = last;
  if (next > INT_MAX) next = INT_MAX;
  return (int32_t)next;
}

// The loop a plan is made for.  terminate == false is the fixed-work loop of Solver::iterate: it stops at iterLim (its
// target) without a check of its own there, and the last iteration of iterLimit is no scheduled check.  Otherwise
// iterLim == iterLimit.
struct RoundLoop {
  int64_t iterLim;
  bool terminate;
  int32_t interval, iterLimit;
  int64_t haltAfter(int64_t it) const {
    // (the fixed-work loop checks nowhere but on the interval — roundEntry, checkDue — so it must not halt at the last
    // iteration of iterLimit either: no check would run there and the device would stay halted in front of its target)
    int64_t h = nextCheckIter((int32_t)it, interval, terminate ? iterLimit : INT_MAX);
    if (!terminate && h > iterLim) h = iterLim;
    return h;
  }
};

// The entry rule: a check is due right at nIter (the device "halts" at the current iteration), or the device runs on to
// the next one.
struct RoundEntry {
  int32_t halted, haltIter;
};
inline RoundEntry roundEntry(int64_t nIter, const RoundLoop& L) {
  const bool onSchedule = nIter < 10 || nIter % L.interval == 0 || (L.terminate && nIter == (int64_t)L.iterLimit - 1);
  return onSchedule ? RoundEntry{1, (int32_t)nIter} : RoundEntry{0, (int32_t)L.haltAfter(nIter)};
}

// The units of the next round from the state record the host holds: the check alone where the device stands halted
// (the entry only: every trial unit is followed by its check), then up to `ahead` units of `todo` trials and a check
// each, every todo the stretch to the next scheduled check under the assumption that every trial is accepted.
struct RoundPlan {
  bool entryCheck = false;
  int32_t nTodo = 0;
  int32_t todo[kRoundMaxUnits];
};
inline RoundPlan planRound(int64_t nIter, int64_t haltIter, bool halted, int32_t ahead, const RoundLoop& L) {
  RoundPlan p;
  int64_t itExp = nIter, haltExp = haltIter;
  if (halted) {
    p.entryCheck = true;
    if (L.terminate && itExp >= L.iterLim - 1) return p;  // the check that ends the solve: nothing is queued behind it
    haltExp = L.haltAfter(itExp);
  }
  int64_t queuedTrials = 0;  // (the tabulated powers of the step rule reach 4096 trials beyond the last refresh)
  for (int32_t u = 0; u < ahead && u < kRoundMaxUnits && queuedTrials < 3000; ++u) {
    int64_t todo = haltExp - itExp;
    if (todo < 1) todo = 1;
    if (todo > kRoundMaxTodo) todo = kRoundMaxTodo;
    p.todo[p.nTodo++] = (int32_t)todo;
    queuedTrials += todo + kRoundSpareTrials;
    itExp = std::min(itExp + todo, haltExp);
    if (itExp >= L.iterLim || (L.terminate && itExp >= L.iterLim - 1)) break;  // the target / the check that ends the solve
    if (itExp == haltExp) haltExp = L.haltAfter(itExp);
  }
  return p;
}

// Queue depth of the next round: doubling from 1, up to ~25 ms of queued work by the clock of the last round (`units`
// units in roundMs), at most 16 units.  sharded: every rank must queue the same units per round — the rounds end in
// collectives — so the depth does not follow this rank's clock there: 1, 2, 4, 4, ...
inline int32_t nextQueueDepth(int32_t ahead, int32_t& aheadMax, int32_t units, double roundMs, bool sharded) {
  if (sharded) aheadMax = 4;
  else if (units > 0 && roundMs > 0.0) aheadMax = std::max(1, std::min(kRoundMaxUnits, (int32_t)(25.0 * units / roundMs)));
  return std::min(ahead * 2, aheadMax);
}

}  // namespace pdlp
