// tools/batch_driver_check.cpp — the batch driver (highs_amd/csrc/pdlp_batch.cpp) behind canned lanes, as a stand-alone
// host program for sanitizer runs (tools/batch_driver_check.sh): no device call is made.  A canned lane "solves" variant k
// in rounds[k] rounds, writes k into R[k].num_iter, and fails where the script says so; the checks are on who solved what,
// the launch counts, the refills and the failure rule.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

#include "pdlp_batch.hpp"

using namespace pdlp;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "FAILED %s:%d: %s\n", __FILE__, __LINE__, #c); exit(1); } } while (0)

namespace {
struct Script {
  std::vector<int> rounds;   // rounds variant k needs
  int failVariant = -1;      // this variant's lane reports a failure in its first round
  std::string sequential;    // lanes' reason for running alone
  int badVariant = -1;       // validate() refuses this variant
};
struct CannedLane : BatchLane {
  const Script& sc;
  int id, variant = -1, left = 0, updates = 0, alone = 0, shared = 0;
  std::vector<int> solved;
  CannedLane(const Script& s, int i) : sc(s), id(i) {}
  std::string sequentialReason() override { return sc.sequential; }
  int32_t workBlocks() override { return 21; }
  void validate(const pdlp_update_t& u) override {
    if (u.reserved == -7) throw std::runtime_error("pdlp_mi355x_update: row 5 would change its kind");
  }
  void setVariant(int32_t k, int32_t) override { variant = k; }
  void update(const pdlp_update_t&) override { ++updates; }
  void runAlone(pdlp_result_t* R) override { R->num_iter = variant; R->num_trials = -1 - id; ++alone; solved.push_back(variant); }
  void begin() override { left = sc.rounds[(size_t)variant]; }
  bool idle() override { return left == 0; }
  void queue(int32_t ahead, std::vector<LaneUnit>& units) override {
    CHECK(ahead >= 1 && ahead <= 16);
    for (int i = 0; i < ahead; ++i) { LaneUnit u; u.hasTrials = true; u.trials.grid = 21; u.check.grid = 21; units.push_back(u); }
    ++shared;
  }
  LaneVerdict afterRound() override {
    if (variant == sc.failVariant) return kLaneFailed;
    return --left <= 0 ? kLaneOver : kLaneGoOn;
  }
  void finish(pdlp_result_t* R) override { R->num_iter = variant; R->num_trials = id; solved.push_back(variant); }
  int32_t xcc() override { return id; }
};
struct CountingBackend : BatchBackend {
  int rounds = 0;
  void round(const std::vector<LaneUnit>* units, int nLanes, int32_t* nt, int32_t* nc) override {
    size_t J = 0;
    for (int l = 0; l < nLanes; ++l) J = std::max(J, units[l].size());
    CHECK(J > 0);
    *nt += (int32_t)J;
    *nc += (int32_t)J;
    ++rounds;
  }
};

void scenario(int nLanes, const Script& sc, int K) {
  std::vector<std::unique_ptr<CannedLane>> own;
  std::vector<BatchLane*> lanes;
  for (int l = 0; l < nLanes; ++l) { own.emplace_back(new CannedLane(sc, l)); lanes.push_back(own.back().get()); }
  CountingBackend be;
  BatchDriver d(lanes, &be);
  std::vector<pdlp_update_t> u((size_t)K);
  std::vector<pdlp_result_t> R((size_t)K);
  memset(u.data(), 0, sizeof(pdlp_update_t) * (size_t)K);
  memset(R.data(), 0, sizeof(pdlp_result_t) * (size_t)K);
  for (auto& r : R) r.num_iter = -1;
  if (sc.badVariant >= 0) {
    u[(size_t)sc.badVariant].reserved = -7;
    bool threw = false;
    try { d.run(K, u.data(), R.data()); } catch (const std::exception& e) {
      threw = true;
      CHECK(std::string(e.what()).find("variant " + std::to_string(sc.badVariant) + ": pdlp_mi355x_update: row 5") == 0);
    }
    CHECK(threw);
    for (auto& l : own) CHECK(l->updates == 0);  // nothing was changed
    for (auto& r : R) CHECK(r.num_iter == -1);
    u[(size_t)sc.badVariant].reserved = 0;
  }
  d.run(K, u.data(), R.data());
  const pdlp_batch_info_t& I = d.info();
  for (int k = 0; k < K; ++k) CHECK(R[(size_t)k].num_iter == k);  // every variant solved, each into its own result
  int solved = 0;
  for (auto& l : own) solved += (int)l->solved.size();
  CHECK(solved == K);  // ... exactly once
  CHECK(I.variants == K && I.lanes == nLanes);
  const bool concurrent = sc.sequential.empty() && nLanes > 1 && K > 1;
  if (!concurrent) {
    CHECK(I.lanes_concurrent == 1 && I.trial_launches == 0 && be.rounds == 0);
    CHECK(strncmp(I.reason, "sequential: ", 12) == 0);
    CHECK((int)own[0]->solved.size() == K);
  } else {
    CHECK(strncmp(I.reason, "concurrent: ", 12) == 0);
    CHECK(I.lanes_concurrent == std::min(nLanes, K));
    CHECK(I.fallback_variants == (sc.failVariant >= 0 && sc.failVariant < K ? 1 : 0));
    if (sc.failVariant >= 0 && sc.failVariant < K) {
      // the failed lane solved its variant alone, after the others, and took part in ONE round only
      const int l = -1 - R[(size_t)sc.failVariant].num_trials;
      CHECK(l >= 0 && l < nLanes && own[(size_t)l]->alone == 1 && own[(size_t)l]->shared == 1);
      CHECK(I.xcc_of_lane[l] == -1);
    }
    CHECK(I.trial_launches == I.check_launches && I.trial_launches > 0);
  }
  printf("ok: %d lanes, K = %d: %s; %d shared launches, %d alone\n", nLanes, K, I.reason, I.trial_launches, I.fallback_variants);
}
}  // namespace

int main() {
  Script a; a.rounds = {3, 1, 4, 1, 5, 9, 2, 6, 5, 3, 5, 8};
  scenario(8, a, 8);
  scenario(3, a, 7);
  scenario(3, a, 12);
  scenario(1, a, 2);
  scenario(8, a, 1);
  Script z = a; z.rounds[2] = 0;  // the iteration limit reached before the first round
  scenario(3, z, 7);
  Script f = a; f.failVariant = 1;
  scenario(3, f, 7);
  scenario(2, f, 12);
  Script s = a; s.sequential = "48 work blocks need more than one XCD";
  scenario(8, s, 3);
  Script b = a; b.badVariant = 2;
  scenario(4, b, 4);
  Script allFail = a; allFail.failVariant = 0;
  scenario(2, allFail, 2);
  printf("batch driver: all scenarios passed\n");
  return 0;
}
