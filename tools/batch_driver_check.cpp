// tools/batch_driver_check.cpp — the batch driver (highs_amd/csrc/pdlp_batch.cpp) behind canned lanes, as a stand-alone
// host program for sanitizer runs (tools/batch_driver_check.sh): no device call is made.  A canned lane "solves" variant k
// in rounds[k] rounds, writes k into R[k].num_iter, and fails where the script says so; the checks are on who solved what,
// the launch counts, the refills and the failure rule.  A canned lane also plays the held solver of a value variant
// (pdlp_mi355x_batch_run_values): it follows which array its "solver" holds through the one update call the lane plans
// (planLaneUpdate), and checks after every update that it holds variant k = P with v[k] applied — whatever it solved
// before, and also after an update that threw half-way.  In DEVICE mode (pdlp_mi355x_batch_run_device) the driver sets the
// mode on every lane, asks lane 0 ONCE for the validation of all variants and results, and the lanes restore from the
// batch's second copy of P — the one that stands for P's data in HBM —, never from the host's: a call never mixes the two.
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
  std::string kinds;         // per variant: n nothing, A a_value, Q q_value, B both, D data (cost and rows); empty: all n
  int throwVariant = -1;     // update() of this variant throws half-way, once
  int disqualifyVariant = -1;  // after this variant's update the lane says it cannot share launches
};
// P of the canned batches, and one set of arrays per variant (their addresses are what the lanes follow)
struct Arrays { std::vector<double> cost{1, 2}, lower{0, 0}, upper{1, 1}, rowLo{0, 0}, rowUp{1, 1}, a{1, 2, 3}, q{4, 5}; };
const int32_t kStart[] = {0, 2, 3}, kIndex[] = {0, 1, 1}, kQStart[] = {0, 1, 2}, kQIndex[] = {0, 1};
pdlp_problem_t problemOf(const Arrays& d) {
  pdlp_problem_t P;
  memset(&P, 0, sizeof(P));
  P.num_col = 2; P.num_row = 2; P.num_nz = 3;
  P.a_start = kStart; P.a_index = kIndex; P.a_value = d.a.data();
  P.col_cost = d.cost.data(); P.col_lower = d.lower.data(); P.col_upper = d.upper.data();
  P.row_lower = d.rowLo.data(); P.row_upper = d.rowUp.data();
  P.q_dim = 2; P.q_start = kQStart; P.q_index = kQIndex; P.q_value = d.q.data();
  return P;
}
const double kTorn = 0.0;  // what an array holds after an update that threw: neither P's nor a variant's
struct Held { const double *cost, *rows, *a, *q; };
struct CannedLane : BatchLane {
  const Script& sc;
  const BaseView base[2];  // P's data where a host call restores from, and where a device call does
  LaneMode mode = kLaneHost;
  int modeSets = 0, hostValidations = 0, deviceValidations = 0, deviceFinishes = 0;
  int id, variant = -1, left = 0, updates = 0, alone = 0, shared = 0, differs = 0, plain = 0, matrix = 0, values = 0;
  bool threw = false, disqualified = false;
  Held held;
  std::vector<int> solved;
  CannedLane(const Script& s, const BaseView& host, const BaseView& device, int i)
      : sc(s), base{host, device}, id(i), held{host.cost, host.rowLower, host.aValue, host.qValue} {}
  const BaseView& mine() const { return base[mode == kLaneDevice ? 1 : 0]; }
  void setMode(LaneMode m) override { mode = m; ++modeSets; }
  std::string sequentialReason() override { return disqualified ? "canned: no longer shareable" : sc.sequential; }
  int32_t workBlocks() override { return 21; }
  void validateDevice(int32_t K, const Variant* v, const pdlp_result_t* R) override {
    CHECK(mode == kLaneDevice && id == 0 && K >= 1 && v && R);
    ++deviceValidations;
    for (int32_t k = 0; k < K; ++k) {
      try {
        refusals(v[k]);
      } catch (const std::exception& e) {
        throw std::runtime_error("variant " + std::to_string(k) + ": " + e.what());
      }
    }
  }
  void validate(const Variant& v) override {
    CHECK(mode == kLaneHost);
    ++hostValidations;
    refusals(v);
  }
  void refusals(const Variant& v) {
    if (v.u.reserved == -7) throw std::runtime_error("pdlp_mi355x_update: row 5 would change its kind");
    if (v.u.reserved == -8) throw std::runtime_error("pdlp_mi355x_update_values: the Hessian is not positive semidefinite");
  }
  void setVariant(int32_t k, int32_t) override { variant = k; }
  // SolverLane::update, with a solver that only remembers whose array it holds
  void update(const Variant& v) override {
    ++updates;
    const LaneUpdatePlan plan = planLaneUpdate(v, differs, mine());
    const Variant& w = plan.v;
    differs |= plan.now;
    CHECK(plan.call == (w.q_value ? kCallUpdateValues : w.a_value ? kCallUpdateMatrix : kCallUpdate));
    CHECK((w.a_value == nullptr) == (w.num_nz == 0) && (w.q_value == nullptr) == (w.num_q_nz == 0));
    if (variant == sc.throwVariant && !threw) {  // half-way: everything it was asked to change is torn
      threw = true;
      if (w.u.col_cost) held.cost = &kTorn;
      if (w.u.row_lower) held.rows = &kTorn;
      if (w.a_value) held.a = &kTorn;
      if (w.q_value) held.q = &kTorn;
      throw std::runtime_error("canned: the update of variant " + std::to_string(variant) + " failed");
    }
    if (w.u.col_cost) held.cost = w.u.col_cost;
    if (w.u.row_lower) { CHECK(w.u.row_upper); held.rows = w.u.row_lower; }
    if (w.a_value) held.a = w.a_value;
    if (w.q_value) held.q = w.q_value;
    differs = plan.now;
    (plan.call == kCallUpdate ? plain : plan.call == kCallUpdateMatrix ? matrix : values)++;
    // variant k = P with v[k] applied
    // ... P's data being the copy that lives where this call's arrays do; what the variant leaves alone and the lane did
    // not differ in stays whichever copy of P it held (both are P)
    auto isP = [&](const double* h, const double* BaseView::*f) { return h == base[0].*f || h == base[1].*f; };
    CHECK(v.u.col_cost ? held.cost == v.u.col_cost : isP(held.cost, &BaseView::cost));
    CHECK(v.u.row_lower ? held.rows == v.u.row_lower : isP(held.rows, &BaseView::rowLower));
    CHECK(v.a_value ? held.a == v.a_value : isP(held.a, &BaseView::aValue));
    CHECK(v.q_value ? held.q == v.q_value : isP(held.q, &BaseView::qValue));
    // a restore made in this call took the copy of this call's side
    if (w.u.col_cost && !v.u.col_cost) CHECK(w.u.col_cost == mine().cost);
    if (w.u.row_lower && !v.u.row_lower) CHECK(w.u.row_lower == mine().rowLower && w.u.row_upper == mine().rowUpper);
    if (w.a_value && !v.a_value) CHECK(w.a_value == mine().aValue && w.num_nz == mine().nnz);
    if (w.q_value && !v.q_value) CHECK(w.q_value == mine().qValue && w.num_q_nz == mine().qSlots);
    if (variant == sc.disqualifyVariant) disqualified = true;
  }
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
  void finish(pdlp_result_t* R) override {
    R->num_iter = variant; R->num_trials = id; solved.push_back(variant);
    deviceFinishes += mode == kLaneDevice ? 1 : 0;
  }
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

void scenario(int nLanes, const Script& sc, int K, bool oldEntry = true, bool device = false) {
  const Arrays p;
  const pdlp_problem_t P = problemOf(p);
  const BaseData base(P), baseInHbm(P);  // (the second stands for the batch's copy of P in HBM: other addresses, never read)
  CHECK(base.aValue.size() == 3 && base.qValue.size() == 2 && base.aValue.data() != p.a.data());  // (a copy: P's arrays may go)
  CHECK(base.view().nnz == 3 && base.view().qSlots == 2 && base.view().cost != baseInHbm.view().cost);
  std::vector<std::unique_ptr<CannedLane>> own;
  std::vector<BatchLane*> lanes;
  for (int l = 0; l < nLanes; ++l) {
    own.emplace_back(new CannedLane(sc, base.view(), baseInHbm.view(), l));
    lanes.push_back(own.back().get());
  }
  CountingBackend be;
  BatchDriver d(lanes, &be);
  std::vector<Arrays> mine((size_t)K);
  std::vector<Variant> u((size_t)K);
  std::vector<pdlp_result_t> R((size_t)K);
  memset(u.data(), 0, sizeof(Variant) * (size_t)K);
  memset(R.data(), 0, sizeof(pdlp_result_t) * (size_t)K);
  int nValue = 0;
  for (int k = 0; k < K; ++k) {
    const char kind = sc.kinds.empty() ? 'n' : sc.kinds[(size_t)k % sc.kinds.size()];
    Arrays& m = mine[(size_t)k];
    Variant& v = u[(size_t)k];
    if (kind == 'A' || kind == 'B') { v.a_value = m.a.data(); v.num_nz = 3; }
    if (kind == 'Q' || kind == 'B') { v.q_value = m.q.data(); v.num_q_nz = 2; }
    if (kind == 'D') { v.u.col_cost = m.cost.data(); v.u.row_lower = m.rowLo.data(); v.u.row_upper = m.rowUp.data(); }
    nValue += hasValues(v) ? 1 : 0;
  }
  const char* entry = device ? kEntryBatchRunDevice : oldEntry ? kEntryBatchRun : kEntryBatchRunValues;
  const LaneMode mode = device ? kLaneDevice : kLaneHost;
  for (auto& r : R) r.num_iter = -1;
  if (sc.badVariant >= 0) {
    u[(size_t)sc.badVariant].u.reserved = oldEntry ? -7 : -8;
    bool threw = false;
    try { d.run(K, u.data(), R.data(), entry, mode); } catch (const std::exception& e) {
      threw = true;
      const char* words = oldEntry ? ": pdlp_mi355x_update: row 5" : ": pdlp_mi355x_update_values: the Hessian is not";
      CHECK(std::string(e.what()).find("variant " + std::to_string(sc.badVariant) + words) == 0);
    }
    CHECK(threw);
    for (auto& l : own) CHECK(l->updates == 0);  // nothing was changed
    for (auto& r : R) CHECK(r.num_iter == -1);
    u[(size_t)sc.badVariant].u.reserved = 0;
  }
  {  // K < 1 and null arrays, by the entry's name
    bool threw = false;
    try { d.run(0, u.data(), R.data(), entry, mode); } catch (const std::exception& e) {
      threw = std::string(e.what()) == std::string(entry) + ": K = 0 variants (at least 1)";
    }
    CHECK(threw);
    threw = false;
    try { d.run(K, nullptr, R.data(), entry, mode); } catch (const std::exception& e) {
      threw = std::string(e.what()) == std::string(entry) + ": null argument";
    }
    CHECK(threw);
  }
  if (sc.throwVariant >= 0) {
    // an update that throws in the middle of a run ends the call; the lanes then differ from P in whatever they were
    // asked to change, so the next call (below) still gives every variant its own arrays
    bool threw = false;
    try { d.run(K, u.data(), R.data(), entry, mode); } catch (const std::exception& e) {
      threw = std::string(e.what()).find("canned: the update of variant") == 0;
    }
    CHECK(threw);
    for (auto& l : own) { l->solved.clear(); l->alone = l->shared = 0; }
    for (auto& r : R) r.num_iter = -1;
  }
  d.run(K, u.data(), R.data(), entry, mode);
  const pdlp_batch_info_t& I = d.info();
  if (device) {
    // a host call first, so that lanes differ from P through HOST arrays when the device call restores them; then the device
    // call again: every lane was told the mode, lane 0 alone validated, once per call, and no lane validated the host's way
    auto again = [&] {
      for (auto& l : own) { l->solved.clear(); l->alone = l->shared = 0; l->disqualified = false; }
    };
    again();
    for (auto& l : own) l->hostValidations = l->deviceValidations = l->deviceFinishes = 0;
    d.run(K, u.data(), R.data(), kEntryBatchRunValues, kLaneHost);
    for (auto& l : own) CHECK(l->mode == kLaneHost && l->deviceValidations == 0 && l->deviceFinishes == 0);
    again();
    CHECK(own[0]->hostValidations == K);
    for (auto& r : R) r.num_iter = -1;
    own[0]->hostValidations = 0;
    d.run(K, u.data(), R.data(), entry, mode);
    for (auto& l : own) CHECK(l->mode == kLaneDevice && l->hostValidations == 0 && l->deviceValidations == (l->id == 0 ? 1 : 0));
  }
  for (int k = 0; k < K; ++k) CHECK(R[(size_t)k].num_iter == k);  // every variant solved, each into its own result
  int solved = 0, plain = 0, valued = 0;
  for (auto& l : own) { solved += (int)l->solved.size(); plain += l->plain; valued += l->matrix + l->values; }
  CHECK(solved == K);  // ... exactly once
  if (nValue == 0) CHECK(valued == 0);  // without value variants every update is the plain one, as before them
  CHECK(valued >= nValue);              // (more: the restores)
  CHECK(I.variants == K && I.lanes == nLanes);
  const bool concurrent = sc.sequential.empty() && nLanes > 1 && K > 1;
  const int fellBack = (sc.failVariant >= 0 && sc.failVariant < K ? 1 : 0) + (sc.disqualifyVariant >= 0 && sc.disqualifyVariant < K ? 1 : 0);
  if (!concurrent) {
    CHECK(I.lanes_concurrent == 1 && I.trial_launches == 0 && be.rounds == 0);
    CHECK(strncmp(I.reason, "sequential: ", 12) == 0);
    CHECK((int)own[0]->solved.size() == K);
  } else {
    CHECK(strncmp(I.reason, "concurrent: ", 12) == 0);
    if (sc.disqualifyVariant < 0) CHECK(I.lanes_concurrent == std::min(nLanes, K));
    CHECK(I.fallback_variants == fellBack);
    if (sc.failVariant >= 0 && sc.failVariant < K) {
      // the failed lane solved its variant alone, after the others, and took part in ONE round only
      const int l = -1 - R[(size_t)sc.failVariant].num_trials;
      CHECK(l >= 0 && l < nLanes && own[(size_t)l]->alone == 1 && own[(size_t)l]->shared == 1);
      CHECK(I.xcc_of_lane[l] == -1);
    }
    if (sc.disqualifyVariant >= 0 && sc.disqualifyVariant < K) {
      // the lane that no longer qualifies after its value update solved that variant alone, and nothing after it
      const int l = -1 - R[(size_t)sc.disqualifyVariant].num_trials;
      CHECK(l >= 0 && l < nLanes && own[(size_t)l]->alone == 1 && own[(size_t)l]->solved.back() == sc.disqualifyVariant);
    }
    CHECK(I.trial_launches == I.check_launches && I.trial_launches > 0);
  }
  printf("ok: %s%d lanes, K = %d%s: %s; %d shared launches, %d alone; %d plain and %d value updates\n", device ? "device mode, " : "", nLanes, K,
         sc.kinds.empty() ? "" : (" [" + sc.kinds + "]").c_str(), I.reason, I.trial_launches, I.fallback_variants, plain, valued);
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
  // value variants: every restore transition on one lane and on two, refills, the sequential classes
  Script v = a; v.kinds = "AnQnBDQn";
  scenario(1, v, 8, false);
  scenario(2, v, 8, false);
  scenario(8, v, 8, false);
  scenario(3, v, 12, false);
  Script vs = v; vs.sequential = "48 work blocks need more than one XCD";
  scenario(8, vs, 8, false);
  Script vb = v; vb.badVariant = 3;
  scenario(4, vb, 8, false);
  // a value variant whose update throws in the middle of a run (a refill on 2 lanes; the first update on 8)
  Script vt = v; vt.throwVariant = 4;
  scenario(2, vt, 8, false);
  scenario(8, vt, 8, false);
  scenario(1, vt, 8, false);
  // a lane that says it no longer qualifies after a value update: the failure rule
  Script vd = v; vd.disqualifyVariant = 2;
  scenario(3, vd, 8, false);
  Script vf = v; vf.failVariant = 1;
  scenario(3, vf, 8, false);
  // device mode: the same driver, the lanes told so per call; restores come from the copy of P that stands for HBM
  scenario(1, v, 8, false, true);
  scenario(2, v, 8, false, true);
  scenario(8, v, 8, false, true);
  scenario(3, v, 12, false, true);
  scenario(8, vs, 8, false, true);
  scenario(4, vb, 8, false, true);
  scenario(2, vt, 8, false, true);
  scenario(3, vd, 8, false, true);
  scenario(3, vf, 8, false, true);
  scenario(3, a, 7, false, true);
  printf("batch driver: all scenarios passed\n");
  return 0;
}
