// pdlp_session.hip — the comparison pass of a session (see pdlp_session.hpp): the caller's arrays of this call, staged in
// HBM, against those of the previous call, kept in HBM.  ONE launch for all arrays.
//
// Every comparison is a pure stream: both sides are read once, unit-stride, with non-temporal loads (neither is read again
// before the update kernels, which stream them too), 16 or 8 bytes per element pair, nothing stored.  Elements are compared
// on their bit patterns (XOR, OR-accumulated in a register), so -0.0 differs from 0.0 and NaNs compare as bits; no
// floating-point operation takes part.  Grid-stride with four independent load pairs in flight per thread and trip; the
// grid is capped, so the record sees at most one atomic OR per wave and one atomicMin per thread that found a row: no
// ordering between threads is needed beyond those two integer atomics.
#include "pdlp_session.hpp"

#include <algorithm>
#include <climits>

#include "pdlp_device.hpp"
#include "pdlp_devfn.hpp"

namespace pdlp {

namespace {

constexpr int kT = 256;
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8 resident blocks of 256 threads; the rest is the grid-stride loop's

// true iff a[i] != b[i] (as bits) for some i = tid, tid + stride, ... < count
template <typename W>
__device__ __forceinline__ bool differs(const W* __restrict__ a, const W* __restrict__ b, int64_t count, int64_t tid, int64_t stride) {
  W acc = 0;
  int64_t i = tid;
  for (; i + 3 * stride < count; i += 4 * stride) {
    const W a0 = ldStream(a + i), a1 = ldStream(a + i + stride), a2 = ldStream(a + i + 2 * stride), a3 = ldStream(a + i + 3 * stride);
    const W b0 = ldStream(b + i), b1 = ldStream(b + i + stride), b2 = ldStream(b + i + 2 * stride), b3 = ldStream(b + i + 3 * stride);
    acc |= (a0 ^ b0) | (a1 ^ b1) | (a2 ^ b2) | (a3 ^ b3);
  }
  for (; i < count; i += stride) acc |= ldStream(a + i) ^ ldStream(b + i);
  return acc != 0;
}

__global__ __launch_bounds__(kT) void k_session_diff(const DiffJobs J, int32_t* record) {
  const int64_t tid = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kT;
  int32_t found = 0;
  for (int k = 0; k < J.nJobs; ++k) {
    const DiffJob& job = J.job[k];
    const bool d = job.width == 8 ? differs((const uint64_t*)job.a, (const uint64_t*)job.b, job.count, tid, stride)
                                  : differs((const uint32_t*)job.a, (const uint32_t*)job.b, job.count, tid, stride);
    if (d) found |= job.bit;
  }
  if (J.rowKind) {  // the rule of k_update_validate (pdlp_update.hip): the smallest row whose kind changes
    int32_t bad = INT_MAX;
    for (int64_t i = tid; i < J.m; i += stride)
      if (rowKindOf(ldStream(J.rowLower + i), ldStream(J.rowUpper + i)) != ldStream(J.rowKind + i)) bad = min(bad, (int32_t)i);
    if (bad != INT_MAX) atomicMin(record + 1, bad);
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) found |= __shfl_xor(found, off, kWave);
  if ((threadIdx.x & (kWave - 1)) == 0 && found) atomicOr(record, found);
}

}  // namespace

void launchSessionDiff(const DiffJobs& jobs, int32_t* record, hipStream_t s) {
  int64_t most = jobs.rowKind ? jobs.m : 0;
  for (int k = 0; k < jobs.nJobs; ++k) most = std::max(most, jobs.job[k].count);
  if (most <= 0) return;
  const int grid = (int)std::min<int64_t>((most + kT - 1) / kT, kMaxBlocks);
  hipLaunchKernelGGL(k_session_diff, dim3(grid), dim3(kT), 0, s, jobs, record);
  PDLP_HIP(hipGetLastError());
}

}  // namespace pdlp
