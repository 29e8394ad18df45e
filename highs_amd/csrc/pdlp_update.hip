// pdlp_update.hip — the device side of pdlp_mi355x_update (see pdlp_update.hpp): new costs, bounds and right-hand sides
// are written in formulated order and taken through the kept scaling passes, in order, with the same single divisions and
// multiplications as k_apply_cols / k_apply_rows (pdlp_setup.hip) and applyScaling (pdlp_host.cpp).  No reductions, no
// float atomics; -ffp-contract=off like every other unit, so host and device agree bit for bit.
//
// Both replay kernels are pure streams: 8 (P + 6) bytes per column, 8 (P + 3) + 8 per row, every byte touched once —
// non-temporal loads and stores.  The pass factors are stored pass-major, so each pass's read is unit-stride across the
// wave; a thread's P loads are independent of each other and of the branch on the column's origin, and are issued first.
#include "pdlp_update.hpp"

#include <algorithm>

#include "pdlp_device.hpp"
#include "pdlp_devfn.hpp"

namespace pdlp {

namespace {

constexpr int kT = 256;
constexpr int kSetupPasses = 11;  // Ruiz x 10 + Pock-Chambolle: the count every scaled cuPDLP-C form has
inline int gridFor(int64_t n) { return (int)((n + kT - 1) / kT); }

__device__ __forceinline__ double infLo(double v) { return v < -1e20 ? -INFINITY : v; }
__device__ __forceinline__ double infUp(double v) { return v > 1e20 ? INFINITY : v; }

__global__ __launch_bounds__(kT) void k_update_validate(const double* __restrict__ rowLower, const double* __restrict__ rowUpper,
                                                        const int32_t* __restrict__ rowKind, int m, int32_t* bad) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= m) return;
  if (rowKindOf(ldStream(rowLower + i), ldStream(rowUpper + i)) != ldStream(rowKind + i)) atomicMin(bad, i);
}

// NP > 0: the pass count is NP (all factor loads in flight before the first division); NP = 0: nPass passes, any count
template <int NP>
__global__ __launch_bounds__(kT) void k_update_cols(int mask, const double* __restrict__ colCost, const double* __restrict__ colLower,
                                                    const double* __restrict__ colUpper, const double* __restrict__ rowLower,
                                                    const double* __restrict__ rowUpper, const int32_t* __restrict__ slackRow,
                                                    double sense, int n0, int n, const double* __restrict__ csPass, int nPass,
                                                    double* cost, double* lower, double* upper) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  double f[NP > 0 ? NP : 1];
  if (NP > 0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) f[p] = ldStream(csPass + (size_t)p * (size_t)n + j);
  }
  bool dc = false, dl = false, du = false;
  double c = 0.0, lo = 0.0, up = 0.0;
  if (j < n0) {
    dc = mask & kUpdCost; dl = mask & kUpdColLower; du = mask & kUpdColUpper;
    if (dc) c = ldStream(colCost + j) * sense;
    if (dl) lo = infLo(ldStream(colLower + j));
    if (du) up = infUp(ldStream(colUpper + j));
  } else if (mask & kUpdRows) {  // slack column of a ranged / free row: its bounds are the row's
    dl = du = true;
    const int r = slackRow[j - n0];
    lo = infLo(rowLower[r]);
    up = infUp(rowUpper[r]);
  }
  if (NP > 0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) { c /= f[p]; lo *= f[p]; up *= f[p]; }
  } else {
    for (int p = 0; p < nPass; ++p) {
      const double cs = ldStream(csPass + (size_t)p * (size_t)n + j);
      c /= cs; lo *= cs; up *= cs;
    }
  }
  if (dc) stStream(cost + j, c);
  if (dl) stStream(lower + j, lo);
  if (du) stStream(upper + j, up);
}

template <int NP>
__global__ __launch_bounds__(kT) void k_update_rows(const double* __restrict__ rowLower, const double* __restrict__ rowUpper,
                                                    const int32_t* __restrict__ rowKind, const int32_t* __restrict__ rowNewIdx, int m,
                                                    const double* __restrict__ rsPass, int nPass, double* rhs) {
  const int i = blockIdx.x * kT + threadIdx.x;
  if (i >= m) return;
  const int ni = ldStream(rowNewIdx + i);  // (0 <= ni < m: a permutation written by formulate)
  const int k = ldStream(rowKind + i);
  const double rl = ldStream(rowLower + i), ru = ldStream(rowUpper + i);
  double f[NP > 0 ? NP : 1];
  if (NP > 0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) f[p] = ldStream(rsPass + (size_t)p * (size_t)m + ni);
  }
  double r;
  if (k == kRowEq) r = rl;
  else if (k == kRowBound) r = 0.0;
  else if (k == kRowLeq) r = -ru;
  else r = rl;
  if (NP > 0) {
#pragma unroll
    for (int p = 0; p < NP; ++p) r /= f[p];
  } else {
    for (int p = 0; p < nPass; ++p) r /= ldStream(rsPass + (size_t)p * (size_t)m + ni);
  }
  stStream(rhs + ni, r);
}

// ---- pdlp_mi355x_update_matrix: refilling a value array of a layout -----------------------------------------------------
// dst[q] = val[src[q]] (src[q] < 0: a pad slot, stays 0).  A pure stream on the store side — 8 B stored and 4 B of index
// loaded per slot, unit-stride, non-temporal — and one gathered 8 B load per slot; val is read once per operand, so it is
// loaded non-temporally too.  Four slots per thread and trip, all index loads, then all gathers, issued before the first
// store; grid-stride.
constexpr int kRefillUnroll = 4;
__global__ __launch_bounds__(kT) void k_refill(const int32_t* __restrict__ src, const double* __restrict__ val, int64_t count,
                                               int64_t nVal, double* __restrict__ dst) {
  const int64_t stride = (int64_t)gridDim.x * kT;
  int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x;
  for (; q + (kRefillUnroll - 1) * stride < count; q += kRefillUnroll * stride) {
    int32_t i[kRefillUnroll];
    double v[kRefillUnroll];
#pragma unroll
    for (int k = 0; k < kRefillUnroll; ++k) i[k] = ldStream(src + q + k * stride);
#pragma unroll
    for (int k = 0; k < kRefillUnroll; ++k) v[k] = (i[k] >= 0 && (int64_t)i[k] < nVal) ? ldStream(val + i[k]) : 0.0;
#pragma unroll
    for (int k = 0; k < kRefillUnroll; ++k) stStream(dst + q + k * stride, v[k]);
  }
  for (; q < count; q += stride) {
    const int32_t i = ldStream(src + q);
    stStream(dst + q, (i >= 0 && (int64_t)i < nVal) ? ldStream(val + i) : 0.0);
  }
}

// Set-up of a matrix-updatable solver: the layouts are built from values that name their own slot (val[q] = q + 1, exact
// in a double), so every value array of a layout then holds, per slot, where its value came from; 0 = a pad.
__global__ __launch_bounds__(kT) void k_tag_values(double* val, int64_t count) {
  for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < count; q += (int64_t)gridDim.x * kT) val[q] = (double)(q + 1);
}
// src[q] = tag - 1 (through `compose` when given), -1 for pads: slots at or beyond nReal, and anything that is no tag
__global__ __launch_bounds__(kT) void k_tags_to_source(const double* __restrict__ tags, int64_t count, int64_t nReal, int64_t nVal,
                                                       const int32_t* __restrict__ compose, int32_t* __restrict__ src,
                                                       unsigned long long* nTagged) {
  unsigned long long mine = 0;
  for (int64_t q = (int64_t)blockIdx.x * kT + threadIdx.x; q < count; q += (int64_t)gridDim.x * kT) {
    const double t = tags[q];
    int32_t i = -1;
    if (q < nReal && t >= 1.0 && t <= (double)nVal && t == (double)(int64_t)t) {
      i = (int32_t)((int64_t)t - 1);
      if (compose) i = compose[i];
      ++mine;
    }
    src[q] = i;
  }
  if (mine) atomicAdd(nTagged, mine);  // (an integer count: order-free)
}

// ---- pdlp_mi355x_update_values: new Hessian values on the kept pattern (pdlp_update.hpp) -------------------------------------
// The assembly map (pdlp_host.hpp HessianMap) is a compact CSR over destinations: j < n the diagonal of column j, n + k
// slot k of qoff.  Sums run in extractHessian's order, one thread per destination, so there is nothing to reduce.

// smallest column whose assembled diagonal is negative (the caller sets bad[0] = n first); reads the staging copy only
__global__ __launch_bounds__(kT) void k_hessian_validate(const int32_t* __restrict__ dstBeg, const int32_t* __restrict__ srcSlot,
                                                         const double* __restrict__ qValue, double sense, int n, int32_t* bad) {
  const int j = blockIdx.x * kT + threadIdx.x;
  if (j >= n) return;
  const int b = ldStream(dstBeg + j), e = ldStream(dstBeg + j + 1);
  double d = 0.0;
  for (int k = b; k < e; ++k) d += qValue[srcSlot[k]] * sense;
  if (d < 0.0) atomicMin(bad, j);
}

// Gathered loads of q_value (a slot is read once or twice: no reuse worth a cache line's stay), unit-stride non-temporal
// stores.  The diagonal accumulates from 0.0; an off-diagonal slot takes its first source and adds the rest.
__global__ __launch_bounds__(kT) void k_hessian_assemble(const int32_t* __restrict__ dstBeg, const int32_t* __restrict__ srcSlot,
                                                         const double* __restrict__ qValue, double sense, int n, int nDst,
                                                         double* __restrict__ qdiag0, double* __restrict__ qoff0) {
  const int d = blockIdx.x * kT + threadIdx.x;
  if (d >= nDst) return;
  const int b = ldStream(dstBeg + d), e = ldStream(dstBeg + d + 1);
  if (d < n) {
    double acc = 0.0;
    for (int k = b; k < e; ++k) acc += ldStream(qValue + srcSlot[k]) * sense;
    stStream(qdiag0 + d, acc);
  } else if (b < e) {  // (every off-diagonal destination has a source: the map is built from the slots)
    double acc = ldStream(qValue + srcSlot[b]) * sense;
    for (int k = b + 1; k < e; ++k) acc += ldStream(qValue + srcSlot[k]) * sense;
    stStream(qoff0 + (d - n), acc);
  }
}

// The scaling passes replayed on the unscaled Hessian: the operations of applyScaling (pdlp_host.cpp) and k_apply_cols
// (pdlp_setup.hip), one pass at a time.  Blocks [0, diagBlocks) take the diagonal — d = (d / cs_p[j]) / cs_p[j], the factor
// unit-stride across the wave — the rest the off-diagonal slots — v = (v / cs_p[row]) / cs_p[col], two gathered 8-byte
// loads per pass.  NP as in k_update_cols: all factor loads in flight before the first division.
template <int NP>
__global__ __launch_bounds__(kT) void k_hessian_replay(const double* __restrict__ qdiag0, const double* __restrict__ qoff0,
                                                       const int32_t* __restrict__ offRow, const int32_t* __restrict__ offCol, int n,
                                                       int nOff, int diagBlocks, const double* __restrict__ csPass, int nPass,
                                                       double* __restrict__ qdiag, double* __restrict__ qoff) {
  if ((int)blockIdx.x < diagBlocks) {
    const int j = blockIdx.x * kT + threadIdx.x;
    if (j >= n) return;
    double f[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) f[p] = ldStream(csPass + (size_t)p * (size_t)n + j);
    }
    double d = ldStream(qdiag0 + j);
    if (NP > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) d = (d / f[p]) / f[p];
    } else {
      for (int p = 0; p < nPass; ++p) {
        const double cs = ldStream(csPass + (size_t)p * (size_t)n + j);
        d = (d / cs) / cs;
      }
    }
    stStream(qdiag + j, d);
  } else {
    const int k = ((int)blockIdx.x - diagBlocks) * kT + threadIdx.x;
    if (k >= nOff) return;
    const int r = ldStream(offRow + k), c = ldStream(offCol + k);  // (0 <= r, c < n: indices of the formulated columns)
    double fr[NP > 0 ? NP : 1], fc[NP > 0 ? NP : 1];
    if (NP > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) { fr[p] = csPass[(size_t)p * (size_t)n + r]; fc[p] = csPass[(size_t)p * (size_t)n + c]; }
    }
    double v = ldStream(qoff0 + k);
    if (NP > 0) {
#pragma unroll
      for (int p = 0; p < NP; ++p) v = (v / fr[p]) / fc[p];
    } else {
      for (int p = 0; p < nPass; ++p) v = (v / csPass[(size_t)p * (size_t)n + r]) / csPass[(size_t)p * (size_t)n + c];
    }
    stStream(qoff + k, v);
  }
}

inline int gridStride(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kT - 1) / kT, 256 * 16)); }

}  // namespace

void launchRefill(const int32_t* src, const double* val, int64_t count, int64_t nVal, double* dst, hipStream_t s) {
  if (count <= 0) return;
  const int64_t perTrip = (int64_t)kT * kRefillUnroll;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((count + perTrip - 1) / perTrip, 256 * 16));
  hipLaunchKernelGGL(k_refill, dim3(grid), dim3(kT), 0, s, src, val, count, nVal, dst);
  PDLP_HIP(hipGetLastError());
}

void launchTagValues(double* val, int64_t count, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_tag_values, dim3(gridStride(count)), dim3(kT), 0, s, val, count);
  PDLP_HIP(hipGetLastError());
}

void launchTagsToSource(const double* tags, int64_t count, int64_t nReal, int64_t nVal, const int32_t* compose, int32_t* src,
                        unsigned long long* nTagged, hipStream_t s) {
  if (count <= 0) return;
  hipLaunchKernelGGL(k_tags_to_source, dim3(gridStride(count)), dim3(kT), 0, s, tags, count, nReal, nVal, compose, src, nTagged);
  PDLP_HIP(hipGetLastError());
}

void launchHessianValidate(const int32_t* dstBeg, const int32_t* srcSlot, const double* qValue, double sense, int32_t n,
                           int32_t* bad, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_hessian_validate, dim3(gridFor(n)), dim3(kT), 0, s, dstBeg, srcSlot, qValue, sense, n, bad);
  PDLP_HIP(hipGetLastError());
}

void launchHessianAssemble(const int32_t* dstBeg, const int32_t* srcSlot, const double* qValue, double sense, int32_t n,
                           int32_t nOff, double* qdiag0, double* qoff0, hipStream_t s) {
  const int64_t nDst = (int64_t)n + nOff;
  if (nDst <= 0) return;
  hipLaunchKernelGGL(k_hessian_assemble, dim3(gridFor(nDst)), dim3(kT), 0, s, dstBeg, srcSlot, qValue, sense, n, (int)nDst, qdiag0,
                     qoff0);
  PDLP_HIP(hipGetLastError());
}

void launchHessianReplay(const double* qdiag0, const double* qoff0, const int32_t* offRow, const int32_t* offCol, int32_t n,
                         int32_t nOff, const double* csPass, int32_t nPass, double* qdiag, double* qoff, hipStream_t s) {
  const int diagBlocks = qdiag0 ? gridFor(n) : 0, offBlocks = qoff0 ? gridFor(nOff) : 0;
  if (diagBlocks + offBlocks <= 0) return;
  const dim3 grid(diagBlocks + offBlocks);
  if (nPass == kSetupPasses)
    hipLaunchKernelGGL(k_hessian_replay<kSetupPasses>, grid, dim3(kT), 0, s, qdiag0, qoff0, offRow, offCol, n, nOff, diagBlocks, csPass,
                       nPass, qdiag, qoff);
  else
    hipLaunchKernelGGL(k_hessian_replay<0>, grid, dim3(kT), 0, s, qdiag0, qoff0, offRow, offCol, n, nOff, diagBlocks, csPass, nPass,
                       qdiag, qoff);
  PDLP_HIP(hipGetLastError());
}

void launchUpdateValidate(const double* rowLower, const double* rowUpper, const int32_t* rowKind, int32_t m, int32_t* bad,
                          hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_update_validate, dim3(gridFor(m)), dim3(kT), 0, s, rowLower, rowUpper, rowKind, m, bad);
  PDLP_HIP(hipGetLastError());
}

void launchUpdateCols(int32_t mask, const double* colCost, const double* colLower, const double* colUpper,
                      const double* rowLower, const double* rowUpper, const int32_t* slackRow, double sense, int32_t n0,
                      int32_t n, const double* csPass, int32_t nPass, double* cost, double* lower, double* upper, hipStream_t s) {
  // only the columns that can change: the originals, and the slack columns when row bounds were given
  const int32_t nDo = (mask & kUpdRows) ? n : ((mask & (kUpdCost | kUpdColLower | kUpdColUpper)) ? n0 : 0);
  if (nDo <= 0) return;
  // (the grid covers nDo columns; a thread beyond them in the last block finds nothing to write)
  const dim3 grid(gridFor(nDo));
  if (nPass == kSetupPasses)
    hipLaunchKernelGGL(k_update_cols<kSetupPasses>, grid, dim3(kT), 0, s, mask, colCost, colLower, colUpper, rowLower, rowUpper,
                       slackRow, sense, n0, n, csPass, nPass, cost, lower, upper);
  else
    hipLaunchKernelGGL(k_update_cols<0>, grid, dim3(kT), 0, s, mask, colCost, colLower, colUpper, rowLower, rowUpper, slackRow,
                       sense, n0, n, csPass, nPass, cost, lower, upper);
  PDLP_HIP(hipGetLastError());
}

void launchUpdateRows(const double* rowLower, const double* rowUpper, const int32_t* rowKind, const int32_t* rowNewIdx,
                      int32_t m, const double* rsPass, int32_t nPass, double* rhs, hipStream_t s) {
  if (m <= 0) return;
  if (nPass == kSetupPasses)
    hipLaunchKernelGGL(k_update_rows<kSetupPasses>, dim3(gridFor(m)), dim3(kT), 0, s, rowLower, rowUpper, rowKind, rowNewIdx, m,
                       rsPass, nPass, rhs);
  else
    hipLaunchKernelGGL(k_update_rows<0>, dim3(gridFor(m)), dim3(kT), 0, s, rowLower, rowUpper, rowKind, rowNewIdx, m, rsPass,
                       nPass, rhs);
  PDLP_HIP(hipGetLastError());
}

}  // namespace pdlp
