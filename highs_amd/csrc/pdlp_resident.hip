// pdlp_resident.hip — the device side of the device-resident entries (see pdlp_resident.hpp): the post-solve of
// Solver::postsolve as two streaming kernels, and the one question about a Hessian in HBM that the host entry answers by
// walking it.  No reductions, no float atomics; -ffp-contract=off like every other unit, and the one place where a product
// feeds a sum (ax * rowScale + x) is spelt with __dmul_rn / __dadd_rn besides, so host and device agree bit for bit.
//
// Both post-solve kernels are pure streams: every result byte is stored once, non-temporally, with vector stores; the loads
// behind the row permutation (ax, y, rowScale at rowNewIdx[i]; the slack column of a ranged row) are 8-byte gathers.
#include "pdlp_resident.hpp"

#include "pdlp_device.hpp"
#include "pdlp_devfn.hpp"

namespace pdlp {

namespace {

constexpr int kT = 256;
inline int gridFor(int64_t n) { return (int)((n + kT - 1) / kT); }

// col_value[j] = x[j] / colScale[j];  col_dual[j] = (slackPos[j] * colScale[j] - slackNeg[j] * colScale[j]) * sense
__global__ __launch_bounds__(kT) void k_postsolve_cols(const double* __restrict__ x, const double* __restrict__ slackPos,
                                                       const double* __restrict__ slackNeg, const double* __restrict__ colScale,
                                                       int n0, int scaled, double sense, double* colValue, double* colDual) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= n0) return;
  const double cs = scaled ? ldStream(colScale + j) : 1.0;
  if (colValue) {
    double v = ldStream(x + j);
    if (scaled) v = v / cs;
    stStream(colValue + j, v);
  }
  if (colDual) {
    double sp = ldStream(slackPos + j), sn = ldStream(slackNeg + j);
    if (scaled) { sp = __dmul_rn(sp, cs); sn = __dmul_rn(sn, cs); }
    stStream(colDual + j, __dmul_rn(__dadd_rn(sp, -sn), sense));
  }
}

// Original row i sits at rowNewIdx[i] of the formulated problem.  row_value: a x un-scaled, negated for a <= row, plus the
// un-scaled slack column n0 + rank for a ranged or free row.  row_dual: y un-scaled, times the sense, negated for a <= row.
__global__ __launch_bounds__(kT) void k_postsolve_rows(const double* __restrict__ ax, const double* __restrict__ y,
                                                       const double* __restrict__ x, const double* __restrict__ rowScale,
                                                       const double* __restrict__ colScale, const int32_t* __restrict__ rowKind,
                                                       const int32_t* __restrict__ rowNewIdx, const int32_t* __restrict__ rowRank,
                                                       int n0, int m, int scaled, double sense, double* rowValue, double* rowDual) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= m) return;
  const int ni = ldStream(rowNewIdx + i);  // (0 <= ni < m: a permutation written by formulate)
  const int k = ldStream(rowKind + i);
  const double rs = scaled ? rowScale[ni] : 1.0;
  if (rowValue) {
    double v = ax[ni];
    if (scaled) v = __dmul_rn(v, rs);
    if (k == kRowLeq) {
      v = -v;
    } else if (k == kRowBound) {
      const int c = n0 + ldStream(rowRank + i);  // (rank < number of ranged-or-free rows = n - n0)
      double xs = x[c];
      if (scaled) xs = xs / colScale[c];
      v = __dadd_rn(v, xs);
    }
    stStream(rowValue + i, v);
  }
  if (rowDual) {
    double d = y[ni];
    if (scaled) d = d / rs;
    d = __dmul_rn(d, sense);
    if (k == kRowLeq) d = -d;
    stStream(rowDual + i, d);
  }
}

// One thread per column of Q walks its slots, as the host's two walks do
__global__ __launch_bounds__(kT) void k_hessian_has_off(const int32_t* __restrict__ qStart, const int32_t* __restrict__ qIndex,
                                                        const double* __restrict__ qValue, int qDim, int everySlot, int32_t* out) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= qDim) return;
  bool any = false;
  for (int p = qStart[j]; p < qStart[j + 1] && !any; ++p) any = qIndex[p] != j && (everySlot || qValue[p] != 0.0);
  if (any) atomicOr(out, 1);
}

}  // namespace

void launchPostsolve(const PostsolveArgs& a, hipStream_t s) {
  if (a.n0 > 0 && (a.colValue || a.colDual))
    hipLaunchKernelGGL(k_postsolve_cols, dim3(gridFor(a.n0)), dim3(kT), 0, s, a.x, a.slackPos, a.slackNeg, a.colScale, a.n0, a.scaled,
                       a.sense, a.colValue, a.colDual);
  if (a.m > 0 && (a.rowValue || a.rowDual))
    hipLaunchKernelGGL(k_postsolve_rows, dim3(gridFor(a.m)), dim3(kT), 0, s, a.ax, a.y, a.x, a.rowScale, a.colScale, a.rowKind,
                       a.rowNewIdx, a.rowRank, a.n0, a.m, a.scaled, a.sense, a.rowValue, a.rowDual);
  PDLP_HIP(hipGetLastError());
}

bool gpuHessianHasOffDiagonal(const int32_t* qStart, const int32_t* qIndex, const double* qValue, int32_t qDim, bool everySlot,
                              hipStream_t s) {
  if (qDim <= 0) return false;
  DeviceArray<int32_t> out;
  out.alloc(1);
  out.zero(s);
  hipLaunchKernelGGL(k_hessian_has_off, dim3(gridFor(qDim)), dim3(kT), 0, s, qStart, qIndex, qValue, qDim, everySlot ? 1 : 0, out.get());
  PDLP_HIP(hipGetLastError());
  int32_t h = 0;
  out.download(&h, 1, s);
  PDLP_HIP(hipStreamSynchronize(s));
  return h != 0;
}

}  // namespace pdlp
