// tools/round_plan_check.cpp — the schedule of a device-driven round (highs_amd/csrc/pdlp_round.hpp) against the
// reference's, as a stand-alone host program for sanitizer runs (tools/round_plan_check.sh): no device call is made.
// The program plays the device: it takes the planner's units round after round and advances its own iteration counter
// the way a persistent launch and a check do.  What it pins the planner on is the reference's rule, restated here and
// nowhere taken from the header: a check stands at iteration `it` exactly when it < 10, it % interval == 0 or
// it == iter_limit - 1 (cupdlp_solver.c:953-962).
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "pdlp_round.hpp"

using namespace pdlp;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace {

struct Case {
  int64_t start;
  int32_t iterLimit, interval, ahead;
  bool terminate;
  int64_t target;  // terminate == false: where the fixed-work loop stops
};

bool refCheckAt(const Case& c, int64_t it) { return it < 10 || it % c.interval == 0 || (c.terminate && it == (int64_t)c.iterLimit - 1); }
int64_t refNextHalt(const Case& c, int64_t it) {  // the next iteration the device halts at
  int64_t h = it + 1;
  // (the fixed-work loop checks nowhere but on the interval, so it must not halt at iter_limit - 1 either: nothing would
  // release it there)
  while (!(h < 10 || h % c.interval == 0 || (c.terminate && h == (int64_t)c.iterLimit - 1))) ++h;
  if (!c.terminate && h > c.target) h = c.target;
  return h;
}

// One loop from c.start to its end.  rejectSeed == 0: every trial is accepted; otherwise every launch loses a
// pseudo-random number of its trials (up to all but one) to rejections.  -> the iterations at which a check ran
std::set<int64_t> drive(const Case& c, unsigned rejectSeed, int64_t* endIter) {
  const int64_t iterLim = c.terminate ? (int64_t)c.iterLimit : c.target;
  const RoundLoop L{iterLim, c.terminate, c.interval, c.iterLimit};
  std::set<int64_t> checks;
  int64_t nIter = c.start;
  CHECK(nIter < iterLim);  // (the callers skip the loops that do not begin)
  const RoundEntry e = roundEntry(nIter, L);
  CHECK((e.halted != 0) == refCheckAt(c, nIter));
  CHECK(e.halted ? e.haltIter == nIter : e.haltIter == refNextHalt(c, nIter));
  if (!c.terminate) CHECK(e.haltIter <= c.target);
  int64_t haltIter = e.haltIter;
  bool halted = e.halted != 0, over = false;
  unsigned rnd = rejectSeed;
  // the device's side of a check: due only where the device stands halted on the schedule; it ends the solve at the
  // last iteration, otherwise it sets the next halt and lets the trials go on
  auto check = [&]() {
    if (!halted || over || (!c.terminate && nIter >= c.target) || !refCheckAt(c, nIter)) return;
    CHECK(checks.insert(nIter).second);
    if (c.terminate && nIter == (int64_t)c.iterLimit - 1) { over = true; return; }
    CHECK(L.haltAfter(nIter) == refNextHalt(c, nIter));
    haltIter = refNextHalt(c, nIter);
    halted = false;
  };
  for (int round = 0;; ++round) {
    CHECK(round < 100000);
    const int64_t iterBefore = nIter;
    const RoundPlan p = planRound(nIter, haltIter, halted, c.ahead, L);
    CHECK(p.entryCheck == halted);
    CHECK(p.entryCheck == (round == 0 && refCheckAt(c, c.start)));  // the first unit is a check alone iff the start is on the schedule
    CHECK(p.nTodo >= 0 && p.nTodo <= c.ahead && p.nTodo <= kRoundMaxUnits);
    if (!halted && p.nTodo > 0) CHECK(p.todo[0] == std::min<int64_t>(kRoundMaxTodo, haltIter - nIter));  // (also behind rejections)
    if (p.entryCheck) check();
    int64_t planned = nIter;
    for (int32_t u = 0; u < p.nTodo; ++u) {
      if (rejectSeed == 0) CHECK(!over);  // nothing is planned behind the check that ends the solve
      const int64_t todo = p.todo[u];
      CHECK(todo >= 1 && todo <= kRoundMaxTodo);
      planned += todo;
      if (!c.terminate) CHECK(planned <= c.target);
      // a persistent launch, stopped by the halt.  All accepted: the todo iterations the plan counts on (where no check
      // falls within a unit's 160 trials a real launch also spends its spare ones and runs ahead of the plan: launches
      // behind the end are no-ops, the next round starts from the state record).  With rejections: todo + spare trials,
      // a pseudo-random number of them lost.
      int64_t accepted = todo;
      if (rejectSeed) {
        rnd = rnd * 1664525u + 1013904223u;
        accepted = todo + kRoundSpareTrials - (int64_t)((rnd >> 8) % (unsigned)(todo + kRoundSpareTrials));
      }
      if (!halted) {
        nIter += std::min(accepted, haltIter - nIter);
        halted = nIter == haltIter;
      }
      check();
    }
    if (rejectSeed == 0 && !over && nIter < iterLim) CHECK(!halted);  // every period has reached its check
    if (over) break;
    if (!c.terminate && nIter >= c.target) break;
    CHECK(nIter > iterBefore || p.entryCheck);  // every round makes progress
  }
  *endIter = nIter;
  return checks;
}

void schedule() {
  const int64_t starts[] = {0, 3, 9, 10, 39, 40, 57};
  const int32_t limits[] = {1, 5, 10, 11, 41, 2000};
  const int32_t intervals[] = {40, 7, 1000};  // (1000: no check within the 160 trials of a unit)
  const int32_t aheads[] = {1, 2, 4, 16};
  int loops = 0;
  for (int64_t start : starts)
    for (int32_t limit : limits)
      for (int32_t interval : intervals)
        for (int32_t ahead : aheads) {
          if (start >= limit) continue;  // the iteration limit is reached before the first round: no loop
          const Case c{start, limit, interval, ahead, true, 0};
          std::set<int64_t> want;
          for (int64_t it = start; it <= (int64_t)limit - 1; ++it)
            if (refCheckAt(c, it)) want.insert(it);
          for (unsigned seed : {0u, 1u, 12345u}) {  // all accepted; with rejections the checks still fall on the schedule
            int64_t end = -1;
            CHECK(drive(c, seed, &end) == want);
            CHECK(end == (int64_t)limit - 1);
          }
          ++loops;
        }
  printf("ok: %d loops end at iter_limit - 1 with their checks exactly on the reference's schedule\n", loops);
}

// a period cut short by rejections: the next round's first unit is what is left of it
void rejections() {
  const RoundLoop L{2000, true, 40, 2000};
  for (int32_t ahead : {1, 2, 4, 16})
    for (int64_t nIter : {41, 57, 79}) {
      const RoundPlan p = planRound(nIter, 80, false, ahead, L);
      CHECK(!p.entryCheck && p.nTodo >= 1 && p.todo[0] == 80 - nIter);
      if (p.nTodo > 1) CHECK(p.todo[1] == 40);
    }
  const RoundLoop far{2000, true, 1000, 2000};  // the 4 * 40 clamp
  const RoundPlan p = planRound(12, 1000, false, 4, far);
  CHECK(p.nTodo == 4 && p.todo[0] == 160 && p.todo[3] == 160);
  printf("ok: the first unit behind a period cut short runs to its halt\n");
}

void fixedWork() {
  int loops = 0;
  for (int64_t start : {0, 3, 9, 10, 39, 40, 57})
    for (int64_t work : {1, 5, 40, 57, 200, 1000})
      for (int32_t interval : {40, 7, 1000})
        for (int32_t ahead : {1, 2, 4, 16})
          // (a finite iteration limit at, one below and well below the target: the loop runs through iter_limit - 1
          // without halting there, where it once stayed halted for good)
          for (int64_t limit : {(int64_t)INT_MAX, start + work, start + work - 1, start + work / 2 + 1}) {
          if (limit < 1) continue;
          const Case c{start, (int32_t)limit, interval, ahead, false, start + work};
          const RoundLoop L{c.target, false, interval, c.iterLimit};
          for (int64_t it = start; it < c.target; ++it) CHECK(L.haltAfter(it) <= c.target && L.haltAfter(it) == refNextHalt(c, it));
          for (unsigned seed : {0u, 7u}) {
            int64_t end = -1;
            const std::set<int64_t> checks = drive(c, seed, &end);
            CHECK(end == c.target);  // no halt lies beyond the target
            for (int64_t it = start; it < c.target; ++it) CHECK((checks.count(it) != 0) == refCheckAt(c, it));
            CHECK(checks.count(c.target) == 0);
          }
          ++loops;
        }
  printf("ok: %d fixed-work loops stop at their target\n", loops);
}

void queueDepth() {
  int32_t ahead = 1, aheadMax = 16;
  const int32_t doubling[] = {2, 4, 8, 16, 16, 16};
  for (int32_t want : doubling) {  // a fast device: doubling from 1 up to the cap
    ahead = nextQueueDepth(ahead, aheadMax, ahead, 0.001, false);
    CHECK(ahead == want && aheadMax == 16);
  }
  ahead = nextQueueDepth(8, aheadMax, 4, 20.0, false);  // 25 ms of work: 25 * 4 / 20 = 5 units
  CHECK(ahead == 5 && aheadMax == 5);
  ahead = nextQueueDepth(2, aheadMax, 8, 12.5, false);  // 16, and doubling still rules below it
  CHECK(ahead == 4 && aheadMax == 16);
  ahead = nextQueueDepth(16, aheadMax, 16, 1.0, false);  // 400: the cap
  CHECK(ahead == 16 && aheadMax == 16);
  ahead = nextQueueDepth(4, aheadMax, 1, 100.0, false);  // 0.25: never below one unit
  CHECK(ahead == 1 && aheadMax == 1);
  aheadMax = 7;
  CHECK(nextQueueDepth(4, aheadMax, 0, 3.0, false) == 7 && aheadMax == 7);  // nothing measured: the depth's bound stays
  CHECK(nextQueueDepth(4, aheadMax, 3, 0.0, false) == 7 && aheadMax == 7);
  ahead = 1;
  aheadMax = 16;
  const int32_t sharded[] = {2, 4, 4, 4};  // (with the first round's 1: 1, 2, 4, 4) whatever this rank's clock says
  for (int32_t want : sharded) {
    ahead = nextQueueDepth(ahead, aheadMax, ahead, ahead == 2 ? 0.001 : 500.0, true);
    CHECK(ahead == want && aheadMax == 4);
  }
  printf("ok: queue depth\n");
}

}  // namespace

int main() {
  schedule();
  rejections();
  fixedWork();
  queueDepth();
  printf("all scenarios passed\n");
  return 0;
}
