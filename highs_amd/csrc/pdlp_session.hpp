// pdlp_session.hpp — a resident solver reused across whole-problem solve calls (pdlp_mi355x_session_*).
//
// The caller passes a whole problem every time.  The session uploads its arrays into the staging buffers the updates
// already use (Solver::updIn_ / updMat_ / updQ_, plus one for the pattern), compares them ON THE DEVICE with the caller's
// arrays of the previous call, which a session-created solver keeps in HBM (pdlp_session.hip: one launch, a record of one
// flag word and the smallest row whose kind changes), and then takes the cheapest of create / update_values /
// update_matrix / update — each of which gives the bits of a fresh create.  The chosen update works from the staged arrays:
// nothing is uploaded twice.  Afterwards staging and kept copies change places, so the kept copy follows without a copy.
//
// The decision itself (what differs -> path, reason) is ONE function, sessionLadder, shared by the session and its host
// twin pdlp_mi355x_host_classify, as rowKindOf is shared by the set-up's two sides.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pdlp_host.hpp"

namespace pdlp {

class Solver;

// What a call found out before it decides.
struct SessionFacts {
  const char* oneShot = nullptr;  // non-null: why this call cannot hold a solver (rule 1)
  bool held = false;              // a solver is held
  int32_t changed = 0;            // PDLP_CHANGED_*
  int32_t kindRow = -1, kindWas = -1, kindNow = -1;
};
// The ladder: path, changed, kind_* and reason of *out from the facts (the timings and held_bytes are the caller's).
void sessionLadder(const SessionFacts& f, pdlp_session_info_t* out);
// Rule 1 from the options and the environment: nullptr, or the reason.
const char* sessionOneShotReason(const pdlp_params_t& opt);
// The option bits of `changed` (structural, run-time) between two calls.
int32_t sessionOptionChanges(const pdlp_params_t& held, const pdlp_params_t& now);
// Slots of the caller's Hessian (0: an LP for the session).
int64_t sessionHessianSlots(const pdlp_problem_t& P);
// What is compared on the host without following an array: sizes, sense, q_dim, Hessian slot count; the offset.
struct SessionShape {
  int32_t numCol = 0, numRow = 0, sense = 0, qDim = 0;
  int64_t nnz = 0, qSlots = 0;
  double offset = 0.0;
};
SessionShape sessionShapeOf(const pdlp_problem_t& P);
int32_t sessionShapeChanges(const SessionShape& held, const SessionShape& now);  // PDLP_CHANGED_SHAPE | PDLP_CHANGED_OFFSET bits

// ---- device (pdlp_session.hip) -------------------------------------------------------------------------------------
// One array pair of the comparison: `count` elements of `width` bytes (8 or 4) compared on their bit patterns; any
// difference ORs `bit` into the record's flag word.
struct DiffJob {
  const void* a = nullptr;
  const void* b = nullptr;
  int64_t count = 0;
  int32_t width = 8;
  int32_t bit = 0;
};
constexpr int kMaxDiffJobs = 12;
struct DiffJobs {
  DiffJob job[kMaxDiffJobs];
  int32_t nJobs = 0;
  // the rows: new bounds against the kept kinds (the rule of k_update_validate); nullptr = no row job
  const double* rowLower = nullptr;
  const double* rowUpper = nullptr;
  const int32_t* rowKind = nullptr;
  int32_t m = 0;
};
// record[0] |= the bits of every job with a difference; record[1] = min(record[1], smallest row whose kind changes).  The
// caller sets record = {0, m} first.  One launch.
void launchSessionDiff(const DiffJobs& jobs, int32_t* record, hipStream_t s);

// ---- the session ------------------------------------------------------------------------------------------------------
class Session {
 public:
  Session();
  ~Session();
  // 0, or the return code of the forwarded pdlp_mi355x_solve (one-shot; its message is already recorded); throws otherwise
  int solve(const pdlp_problem_t& P, const pdlp_params_t& opt, pdlp_result_t* R);
  void release() noexcept;
  const pdlp_session_info_t& info() const { return info_; }

 private:
  void create(const pdlp_problem_t& P, const pdlp_params_t& opt);
  void findChanges(const pdlp_problem_t& P, const pdlp_params_t& opt, SessionFacts& f);
  void applyReuse(const pdlp_problem_t& P, const pdlp_params_t& opt, int32_t changed);
  Solver* solver_ = nullptr;
  pdlp_params_t heldOpt_{};  // the caller's options of the call that left solver_ as it is
  SessionShape held_;        // of the held problem
  pdlp_session_info_t info_{};
};

}  // namespace pdlp
