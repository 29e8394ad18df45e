// pdlp_resident.hpp — the device-resident entries (pdlp_mi355x_create_device, _update_device, _run_device): problems,
// updates and solutions as arrays that are in HBM on the solver's device already.
//
// Nothing new is computed here.  create_device is the device-side set-up (pdlp_setup.hip) without its uploads;
// update_device is the three updates (pdlp_update.cpp) with the staging copy made device to device; run_device is run()
// with the post-solve as kernels.  What the host still needs of the caller's arrays — the starts for the monotone checks,
// costs and row bounds for the left-to-right norms, a hot start — is downloaded into a host shadow: O(n + m), never the
// matrix or the Hessian.
//
// THE POINTER CHECK: every array pointer a device entry is given goes through requireDevicePointer before the first
// launch or copy.  A host pointer must never reach a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>
#include <vector>

#include "pdlp_setup.hpp"
#include "pdlp_update.hpp"

namespace pdlp {

constexpr const char* kEntryCreateDevice = "pdlp_mi355x_create_device";
constexpr const char* kEntryUpdateDevice = "pdlp_mi355x_update_device";
constexpr const char* kEntryRunDevice = "pdlp_mi355x_run_device";

// Throws "<field> is not device memory on device <d>" unless p is NULL or points into memory allocated on device d
// (hipPointerGetAttributes: hipMemoryTypeDevice, not managed, that device).  Pageable host memory makes the query fail:
// that is "not device memory" too, and the runtime's sticky error is cleared.  Launches nothing, copies nothing.
void requireDevicePointer(const void* p, const char* field, int device);
// ... every array of a problem / an update / a result in turn, in the order of the struct's fields
void requireDeviceProblem(const pdlp_problem_t& P, int device);
void requireDeviceUpdate(const double* aValue, const double* qValue, const pdlp_update_t* u, int device);
void requireDeviceResult(const pdlp_result_t& R, int device);

// What create_device refuses of the struct alone, before any HIP call: the null arrays validateProblem names, in its words
// (the starts themselves are checked once their host copy exists).
void residentProblemShape(const pdlp_problem_t& P);

// The route of an update_device call, as pdlp_mi355x_batch_run_values routes a variant, and what that host entry refuses
// before it looks at a value — in its order and words, from facts the host holds.  No HIP call.
enum ResidentRoute { kRouteUpdate, kRouteUpdateMatrix, kRouteUpdateValues };
ResidentRoute residentRoute(int32_t updatable, const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz);
void residentUpdateRefusal(const ValueUpdateFacts& f, const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz,
                           const pdlp_update_t& u);

// A problem whose arrays are in HBM, and its host shadow.
struct ResidentProblem {
  pdlp_problem_t shadow{};  // sizes, scalars; host copies of a_start, col_cost, row_lower, row_upper, q_start, start_*;
                            // every other array: the caller's pointer into HBM (asked only whether it is NULL)
  DeviceInputs in;          // the caller's arrays as the set-up's kernels read them
  DeviceHessianInputs hess;
  hipStream_t callerStream = nullptr;
  std::vector<int32_t> hStart, hQStart;
  std::vector<double> hCost, hRowLower, hRowUpper, hStartCol, hStartRow, hStartDual;

  ResidentProblem(const pdlp_problem_t& Pdev, hipStream_t caller);
  // orders s behind the caller's stream, then downloads the shadow's arrays on s; synchronises
  void fetchShadow(hipStream_t s);
  // hessianHasOffDiagonal / hessianHasOffDiagonalSlot (pdlp_host.hpp) by a kernel; also refuses a Hessian that only the
  // host walk can extract (q_start malformed, PDLP_MI355X_GPU_HESSIAN=0).  After fetchShadow.
  bool hasOffDiagonalHessian(bool everySlot, bool switchOn, hipStream_t s);
};

// s waits for everything enqueued on `caller` so far (an event recorded there; the caller's stream is never synchronised).
// caller == nullptr is the default stream.
void orderBehind(hipStream_t s, hipStream_t caller);

// ---- device (pdlp_resident.hip) --------------------------------------------------------------------------------------
// out[0] = 1 if some slot (row != column) counts: every such slot (everySlot), else those with a non-zero value
bool gpuHessianHasOffDiagonal(const int32_t* qStart, const int32_t* qIndex, const double* qValue, int32_t qDim, bool everySlot,
                              hipStream_t s);
// Solver::postsolve's loops (PDHG_PostSolve: un-scale, un-permute, un-negate) on vectors in HBM, operation for operation.
struct PostsolveArgs {
  const double *x, *slackPos, *slackNeg, *y, *ax;  // formulated, scaled: the iterate run() returns
  const double *colScale, *rowScale;
  const int32_t *rowKind, *rowNewIdx, *rowRank;    // per original row; rank among the ranged-or-free rows
  int32_t n0, m, scaled;
  double sense;
  double *colValue, *colDual, *rowValue, *rowDual;  // each may be nullptr: skipped
};
void launchPostsolve(const PostsolveArgs& a, hipStream_t s);

}  // namespace pdlp
