// pdlp_halpern_small.hpp — the Halpern steps kFirst..kLast of a block as ONE persistent launch on small LPs
// (pdlp_halpern_small.hip), and the rule that says which solvers take it.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "pdlp_kernels.hpp"

namespace pdlp {

// ---- qualification (pure host logic: no device, no solver) --------------------------------------------------------------
// Why a HiPDLP solver keeps its two plain launches per step; 0 = its steps 2..40 run as the persistent launch.
enum : int32_t {
  kHsPersistent = 0,
  kHsSwitchOff = 1,      // PDLP_MI355X_PERSISTENT_HIPDLP=0
  kHsSharded = 2,
  kHsProfile = 3,        // stage "profile_on": eager launches between events
  kHsSlab = 4,           // an operand is in the slab layout
  kHsNot512 = 5,         // an operand does not stream in 512-entry blocks
  kHsLongMajor = 6,      // an operand has a major longer than a block (segment tasks)
  kHsTooManyBlocks = 7,  // more than kHalpernSmallMaxBlocks work blocks
  kHsNotResident = 8,    // the device does not hold the launch's workgroups at once
};
constexpr int32_t kHalpernSmallMaxBlocks = 64;    // the flat sweep barrier's range (beyond it: the hierarchical one, not built here)
constexpr int32_t kHalpernSmallLocalBlocks = 32;  // one XCD has 32 CUs: up to one workgroup per CU the XCD-local mode is taken
struct HalpernSmallShape {
  int32_t blocksA, blocksAt;      // stream work blocks of A (by rows) and A' (by columns)
  int32_t chunkA, chunkAt;        // their work plans' block size
  int32_t useSlab;                // either operand is in the slab layout
  int32_t longTasks;              // segment tasks of long majors, both operands
  int32_t longContrib;            // either operand sums its long majors' contributions in groups
  int32_t sharded, profile, switchOn;
  int32_t resident;               // workgroups of the kernel the device keeps resident at once (halpernSmallResident)
};
// the launch's working workgroups: a workgroup beyond an operand's blocks only meets the barriers
inline int32_t halpernSmallGrid(const HalpernSmallShape& s) { return s.blocksA > s.blocksAt ? s.blocksA : s.blocksAt; }
inline int32_t halpernSmallReason(const HalpernSmallShape& s) {
  if (!s.switchOn) return kHsSwitchOff;
  if (s.sharded) return kHsSharded;
  if (s.profile) return kHsProfile;
  if (s.useSlab) return kHsSlab;
  if (s.chunkA != kChunkSmall || s.chunkAt != kChunkSmall || s.blocksA <= 0 || s.blocksAt <= 0) return kHsNot512;
  if (s.longTasks > 0 || s.longContrib) return kHsLongMajor;
  if (halpernSmallGrid(s) > kHalpernSmallMaxBlocks) return kHsTooManyBlocks;
  if (halpernSmallGrid(s) > s.resident) return kHsNotResident;
  return kHsPersistent;
}
// 1: XCD-local (every eighth workgroup of 8 * grid works), 0: agent-scope accesses on all XCDs
inline int32_t halpernSmallMode(int32_t grid, bool xcdLocalAllowed) { return grid <= kHalpernSmallLocalBlocks && xcdLocalAllowed ? 1 : 0; }

// ---- the launch ---------------------------------------------------------------------------------------------------------
// Words of the barrier buffer.  [0, 4 grid + 16) are zeroed by a memset in front of EVERY launch: arrival words, timeout
// flag, roll-call word, XCC ids, the self-test's words.  The two words behind them live as long as the solver.
constexpr size_t kHsKeepWord = 4 * (size_t)kHalpernSmallMaxBlocks + 16;
constexpr size_t kHsTestedWord = kHsKeepWord;      // XCD-local mode: the nt-load self-test has passed on this solver
constexpr size_t kHsForceWord = kHsKeepWord + 1;   // stage "stall_next_block": the next launch reports this stall code and does nothing
constexpr size_t kHalpernSmallBarWords = kHsKeepWord + 8;
inline size_t halpernSmallZeroedWords(int32_t grid) { return 4 * (size_t)grid + 16; }

struct HalpernSmallLaunch {
  MatView A, At;
  HalpernVecs h{};                 // kOff / major are the launch's business
  HalpernState* st = nullptr;
  unsigned long long* bar = nullptr;  // kHalpernSmallBarWords words, zeroed once by the owner
  int32_t grid = 0;
  int32_t kFirst = 2, kLast = 40;  // k_offset of the first and of the last (major) step
  int32_t timeoutMs = 1000;
};
// Workgroups of k_halpern_small the device keeps resident (capped as smallTrialsGrid caps the trial loop's); 0: unknown
int halpernSmallResident(int device);
// The memset of the per-launch words and the launch, on stream s (both are captured where s is being captured).
void launchHalpernSmall(const HalpernSmallLaunch& q, int mode, hipStream_t s);

}  // namespace pdlp
