// tools/pool_driver_check.cpp — the pool driver (highs_amd/csrc/pdlp_pool.cpp) behind canned lanes, as a stand-alone host
// program for sanitizer runs (tools/pool_driver_check.sh): no device call is made.  A canned solver "solves" problem k in
// rounds[k] rounds and writes k into R[k].num_iter; the script says which problems do not qualify, whose lane fails, and
// which create or solve throws.  The checks are on who solved what and how, the number of solvers alive, the launch counts,
// the refills and the failure rule.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <stdexcept>

#include "pdlp_pool.hpp"

using namespace pdlp;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace {
struct Script {
  std::vector<int> rounds;      // rounds problem k needs
  std::set<int> alone;          // these problems' solvers do not qualify
  std::set<int> threeBarriers;  // these problems' loops keep the P phase
  int failProblem = -1;         // this problem's lane reports a failure in its first round
  int throwCreate = -1;         // this problem's create throws
  int throwSolve = -1;          // this problem's solve throws in its second round (or in its run alone)
};
struct World {
  const Script& sc;
  int alive = 0, mostAlive = 0, created = 0, rounds = 0;
  std::vector<int> order;  // problems in the order of their creates
  explicit World(const Script& s) : sc(s) {}
};
struct CannedLane : PoolLane {
  World& w;
  int k, left = 0, roundsSeen = 0, shared = 0;
  CannedLane(World& w_, int k_) : w(w_), k(k_) { w.mostAlive = std::max(w.mostAlive, ++w.alive); }
  ~CannedLane() override { --w.alive; }
  std::string sequentialReason() override {
    return w.sc.alone.count(k) ? std::to_string(40 + k) + " work blocks need more than one XCD" : std::string();
  }
  void runAlone(pdlp_result_t* R) override {
    if (k == w.sc.throwSolve) throw std::runtime_error("the adaptive step-size search does not terminate");
    R->num_iter = k;
    R->num_trials = -1;
  }
  void begin() override { left = w.sc.rounds[(size_t)k]; }
  bool idle() override { return left == 0; }
  void queue(int32_t ahead, std::vector<LaneUnit>& units) override {
    CHECK(ahead >= 1 && ahead <= 16);
    for (int i = 0; i < ahead; ++i) {
      LaneUnit u;
      u.hasTrials = true;
      u.trials.grid = 1 + k % 32;
      u.trials.primalInA = !w.sc.threeBarriers.count(k);
      u.check.grid = 1 + k % 32;
      units.push_back(u);
    }
    ++shared;
  }
  LaneVerdict afterRound() override {
    ++roundsSeen;
    if (k == w.sc.failProblem) return kLaneFailed;
    if (k == w.sc.throwSolve && roundsSeen == 2) throw std::runtime_error("the adaptive step-size search does not terminate");
    return --left <= 0 ? kLaneOver : kLaneGoOn;
  }
  void finish(pdlp_result_t* R) override { R->num_iter = k; R->num_trials = shared; }
  int32_t xcc() override { return 7 - k % 8; }
};
struct CannedBackend : PoolBackend {
  World& w;
  int nLanes;
  CannedBackend(World& w_, int n) : w(w_), nLanes(n) {}
  std::unique_ptr<PoolLane> create(int32_t k) override {
    CHECK(w.alive <= nLanes);  // at most `lanes` solvers exist while one more is created
    if (k == w.sc.throwCreate) throw std::runtime_error("null column arrays");
    w.order.push_back(k);
    ++w.created;
    return std::unique_ptr<PoolLane>(new CannedLane(w, k));
  }
  void round(const std::vector<LaneUnit>* units, PoolLane* const* lanes, int n, int32_t* nt, int32_t* nc, int32_t* nm) override {
    CHECK(n == nLanes);
    size_t J = 0;
    for (int l = 0; l < n; ++l) {
      CHECK(units[l].empty() == (lanes[l] == nullptr));  // a lane with a solver has queued, an empty one has not
      J = std::max(J, units[l].size());
    }
    CHECK(J > 0);
    for (size_t j = 0; j < J; ++j) {
      int two = 0, three = 0;
      for (int l = 0; l < n; ++l)
        if (j < units[l].size()) ++(units[l][j].trials.primalInA ? two : three);
      if (two && three) ++*nm;
    }
    *nt += (int32_t)J;
    *nc += (int32_t)J;
    ++w.rounds;
  }
};

void scenario(const char* what, int nLanes, const Script& sc, int K) {
  World w(sc);
  CannedBackend be(w, nLanes);
  PoolDriver d(nLanes, &be);
  std::vector<pdlp_result_t> R((size_t)K);
  std::vector<int32_t> path((size_t)K, 77);
  memset(R.data(), 0, sizeof(pdlp_result_t) * (size_t)K);
  for (auto& r : R) r.num_iter = -1;
  const int thrower = sc.throwCreate >= 0 ? sc.throwCreate : sc.throwSolve;
  bool threw = false;
  try {
    d.run(K, R.data(), path.data());
  } catch (const std::exception& e) {
    threw = true;
    CHECK(thrower >= 0);
    const std::string want = "problem " + std::to_string(thrower) + ": " +
                             (sc.throwCreate >= 0 ? "null column arrays" : "the adaptive step-size search does not terminate");
    CHECK(e.what() == want);
  }
  const pdlp_pool_info_t& I = d.info();
  CHECK(w.alive == 0);  // every solver is destroyed, on every way out
  CHECK(w.mostAlive <= nLanes);  // (a lane is free before its next solver is created)
  CHECK(I.problems == K && I.lanes == nLanes);
  for (size_t i = 0; i < w.order.size(); ++i) CHECK(w.order[i] == (int)i);  // the caller's order
  if (thrower >= 0 && thrower < K) {
    CHECK(threw);
    // what was finished stays valid and is marked; what was not is marked as not run
    for (int k = 0; k < K; ++k) {
      if (path[(size_t)k] != PDLP_POOL_NOT_RUN) CHECK(R[(size_t)k].num_iter == k);
      else CHECK(R[(size_t)k].num_iter == -1);
    }
    CHECK(path[(size_t)thrower] == PDLP_POOL_NOT_RUN);
    printf("ok: %s: %d lanes, K = %d: threw for problem %d, %d solvers created\n", what, nLanes, K, thrower, w.created);
    return;
  }
  CHECK(!threw);
  CHECK(w.created == K);
  for (int k = 0; k < K; ++k) CHECK(R[(size_t)k].num_iter == k);  // every problem solved, each into its own result
  int nShared = 0, nAlone = 0, nFall = 0;
  for (int k = 0; k < K; ++k) {
    const int32_t p = path[(size_t)k];
    nShared += p == PDLP_POOL_SHARED; nAlone += p == PDLP_POOL_ALONE; nFall += p == PDLP_POOL_FALLBACK;
    CHECK(p != PDLP_POOL_NOT_RUN && p != 77);
  }
  CHECK(nShared == I.shared_problems && nAlone == I.alone_problems && nFall == I.fallback_problems);
  CHECK(nShared + nAlone + nFall == K);
  const bool concurrent = nLanes > 1 && K > 1;
  if (!concurrent) {
    CHECK(I.lanes_concurrent == 1 && I.trial_launches == 0 && I.check_launches == 0 && I.mixed_launches == 0 && w.rounds == 0);
    CHECK(nAlone == K && w.mostAlive == 1);
    CHECK(strncmp(I.reason, "sequential: ", 12) == 0);
  } else {
    int qualifying = 0, firstAlone = -1;
    for (int k = 0; k < K; ++k) {
      if (sc.alone.count(k)) {
        CHECK(path[(size_t)k] == PDLP_POOL_ALONE && R[(size_t)k].num_trials == -1);
        if (firstAlone < 0) firstAlone = k;
      } else {
        ++qualifying;
      }
    }
    if (firstAlone >= 0) CHECK(I.reason == std::to_string(40 + firstAlone) + " work blocks need more than one XCD");
    else CHECK(strncmp(I.reason, "concurrent: ", 12) == 0);
    const bool fails = sc.failProblem >= 0 && sc.failProblem < K;
    if (fails) {
      // the failed lane's problem was solved alone, after one shared round, and the lane took nothing afterwards
      CHECK(path[(size_t)sc.failProblem] == PDLP_POOL_FALLBACK && R[(size_t)sc.failProblem].num_trials == -1);
      CHECK(nFall >= 1);
    } else {
      CHECK(nFall == 0 && nShared == qualifying);
      CHECK(I.lanes_concurrent == std::min(nLanes, qualifying) || qualifying == 0);
    }
    if (qualifying > 0) CHECK(I.trial_launches == I.check_launches && I.trial_launches > 0);
    bool anyThree = false, anyTwo = false;
    for (int k = 0; k < K; ++k)
      if (!sc.alone.count(k)) (sc.threeBarriers.count(k) ? anyThree : anyTwo) = true;
    if (!(anyThree && anyTwo)) CHECK(I.mixed_launches == 0);
    CHECK(I.mixed_launches <= I.trial_launches);
  }
  printf("ok: %s: %d lanes, K = %d: %s; %d shared launches (%d mixed), %d shared, %d alone, %d fallback, at most %d solvers\n", what,
         nLanes, K, I.reason, I.trial_launches, I.mixed_launches, nShared, nAlone, nFall, w.mostAlive);
}
}  // namespace

int main() {
  Script a; a.rounds = {3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8, 9, 7, 9, 3};
  scenario("full lanes", 8, a, 8);
  scenario("refills, uneven ends", 3, a, 9);
  scenario("refills, uneven ends", 3, a, 16);
  scenario("one lane", 1, a, 3);
  scenario("one problem", 8, a, 1);
  Script z = a; z.rounds[2] = 0;  // the iteration limit reached before the first round
  scenario("an idle problem", 3, z, 7);
  Script n = a; n.alone = {4};
  scenario("a non-qualifying problem in the middle", 3, n, 9);
  Script n2 = a; n2.alone = {0, 1, 2, 8};
  scenario("non-qualifying problems first and last", 3, n2, 9);
  Script all = a; for (int k = 0; k < 16; ++k) all.alone.insert(k);
  scenario("nothing qualifies", 4, all, 5);
  Script m = a; m.threeBarriers = {1, 6};
  scenario("mixed barriers", 8, m, 8);
  {
    World w(m); CannedBackend be(w, 8); PoolDriver d(8, &be);
    std::vector<pdlp_result_t> R(8); std::vector<int32_t> path(8);
    memset(R.data(), 0, sizeof(pdlp_result_t) * 8);
    d.run(8, R.data(), path.data());
    CHECK(d.info().mixed_launches > 0);  // problem 1 (1 round) and problem 6 (2 rounds) ride with two-barrier lanes
    CHECK(d.info().mixed_launches < d.info().trial_launches);  // ... and once both have ended the launches are uniform again
  }
  Script f = a; f.failProblem = 1;
  scenario("the failure rule", 3, f, 7);
  scenario("the failure rule", 2, f, 12);
  Script allFail = a; allFail.failProblem = 0;
  scenario("every lane but one fails", 2, allFail, 2);
  Script tc = a; tc.throwCreate = 5;
  scenario("a create throws mid-run", 3, tc, 9);
  Script ts = a; ts.throwSolve = 4;
  scenario("a solve throws mid-run", 3, ts, 9);
  Script ta = a; ta.alone = {4}; ta.throwSolve = 4;
  scenario("a run alone throws", 3, ta, 9);
  scenario("a solve throws, one lane", 1, ts, 6);
  printf("pool driver: all scenarios passed\n");
  return 0;
}
