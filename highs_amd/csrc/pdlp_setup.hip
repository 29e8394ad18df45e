// pdlp_setup.hip — GPU-side formulate / scale / transpose / slab layout (see pdlp_setup.hpp).
// One-off streaming passes and rocPRIM radix sorts; everything order-sensitive is
// done by one thread per major in the reference's traversal order so that the
// result is bit-identical to the host path and to the reference.
#include "pdlp_setup.hpp"
#include "pdlp_update.hpp"

#include <cstring>

#include <rocprim/rocprim.hpp>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <limits>

namespace pdlp {

namespace {

constexpr int kT = 256;
inline int gridFor(int64_t n) { return (int)std::max<int64_t>(1, std::min<int64_t>((n + kT - 1) / kT, 65535 * 16)); }
#define GSTRIDE(i, n) for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (int64_t)gridDim.x * blockDim.x)

constexpr double kBoundInf = 1e20;

// ---- formulate -----------------------------------------------------------------
// infThresh / freeKind: 1e20 and kRowBound on the cuPDLP-C path (CupdlpWrapper.cpp:316-343); +inf and
// kRowFree on the HiPDLP path (pdhg.cc:175-197)
__device__ __forceinline__ bool isEqKind(int k) { return k == kRowEq || k == kRowBound || k == kRowFree; }
__global__ void k_row_classify(const double* __restrict__ lo, const double* __restrict__ up, int m, double infThresh,
                               int freeKind, int32_t* kind, int32_t* eqFlag, int32_t* ineqFlag, int32_t* slackFlag) {
  GSTRIDE(i, m) {
    const bool hl = lo[i] > -infThresh, hu = up[i] < infThresh;
    int k;
    if (hl && hu && lo[i] == up[i]) k = kRowEq;
    else if (hl && !hu) k = kRowGeq;
    else if (!hl && hu) k = kRowLeq;
    else if (hl && hu) k = kRowBound;  // ranged: a'x - z = 0 with a bounded slack
    else k = freeKind;                 // free: the same, unbounded slack
    kind[i] = k;
    eqFlag[i] = isEqKind(k) ? 1 : 0;
    ineqFlag[i] = (k == kRowLeq || k == kRowGeq) ? 1 : 0;
    slackFlag[i] = (k == kRowBound || k == kRowFree) ? 1 : 0;
  }
}

__device__ __forceinline__ double clampInfLo(double v) { return v < -kBoundInf ? -INFINITY : v; }
__device__ __forceinline__ double clampInfUp(double v) { return v > kBoundInf ? INFINITY : v; }

__global__ void k_row_finish(const double* __restrict__ lo, const double* __restrict__ up, const int32_t* kind,
                             const int32_t* eqRank, const int32_t* ineqRank, const int32_t* slackRank, int m, int n0,
                             int nEq, int64_t nnz0, int32_t* rowNewIdx, double* rhs, double* cost, double* lower,
                             double* upper, int32_t* cscBeg, int32_t* cscIdx, int32_t* cscCol, double* cscVal,
                             double* rowUpper /* HiPDLP form only, else nullptr */) {
  GSTRIDE(i, m) {
    const int k = kind[i];
    const int ni = isEqKind(k) ? eqRank[i] : nEq + ineqRank[i];
    rowNewIdx[i] = ni;
    double r;
    if (k == kRowEq) r = lo[i];
    else if (k == kRowBound || k == kRowFree) r = 0.0;
    else if (k == kRowLeq) r = -up[i];
    else r = lo[i];
    rhs[ni] = r;
    if (rowUpper) rowUpper[ni] = (k == kRowEq) ? up[i] : ((k == kRowBound || k == kRowFree) ? 0.0 : INFINITY);
    if (k == kRowBound || k == kRowFree) {
      const int j = n0 + slackRank[i];
      cost[j] = 0.0;
      lower[j] = rowUpper ? lo[i] : clampInfLo(lo[i]);
      upper[j] = rowUpper ? up[i] : clampInfUp(up[i]);
      const int64_t p = nnz0 + slackRank[i];
      cscBeg[j] = (int32_t)p;
      cscIdx[p] = ni;
      cscCol[p] = j;
      cscVal[p] = -1.0;
    }
  }
}

__global__ void k_col_setup(const double* __restrict__ c, const double* __restrict__ lo, const double* __restrict__ up,
                            const int32_t* __restrict__ aStart, int n0, double sense, int clampInf, double* cost,
                            double* lower, double* upper, int32_t* cscBeg) {
  GSTRIDE(j, n0) {
    cost[j] = c[j] * sense;
    lower[j] = clampInf ? clampInfLo(lo[j]) : lo[j];
    upper[j] = clampInf ? clampInfUp(up[j]) : up[j];
    cscBeg[j] = aStart[j];
  }
}

// Reference entry order inside a column: equality-type rows first, then inequality rows (LEQ negated).
// VALS_ONLY (pdlp_mi355x_update_matrix: the pattern was checked and written at set-up): cscVal alone.
template <bool VALS_ONLY>
__global__ void k_col_entries(const int32_t* __restrict__ aStart, const int32_t* __restrict__ aIndex,
                              const double* __restrict__ aValue, const int32_t* __restrict__ kind,
                              const int32_t* __restrict__ rowNewIdx, int n0, int m, int32_t* cscIdx, int32_t* cscCol,
                              double* cscVal, int32_t* badFlag) {
  GSTRIDE(j, n0) {
    const int b = aStart[j], e = aStart[j + 1];
    int k = b;
    for (int p = b; p < e; ++p) {
      const int r = aIndex[p];
      if (r < 0 || r >= m) { if (!VALS_ONLY) *badFlag = 1; continue; }
      const int t = kind[r];
      if (isEqKind(t)) { if (!VALS_ONLY) { cscIdx[k] = rowNewIdx[r]; cscCol[k] = (int)j; } cscVal[k] = aValue[p]; ++k; }
    }
    for (int p = b; p < e; ++p) {
      const int r = aIndex[p];
      if (r < 0 || r >= m) continue;
      const int t = kind[r];
      if (t == kRowLeq) { if (!VALS_ONLY) { cscIdx[k] = rowNewIdx[r]; cscCol[k] = (int)j; } cscVal[k] = -aValue[p]; ++k; }
      else if (t == kRowGeq) { if (!VALS_ONLY) { cscIdx[k] = rowNewIdx[r]; cscCol[k] = (int)j; } cscVal[k] = aValue[p]; ++k; }
    }
  }
}

// ---- transposes ----------------------------------------------------------------
__global__ void k_iota(int32_t* a, int64_t n) { GSTRIDE(i, n) a[i] = (int32_t)i; }
__global__ void k_fill_d(double* a, double v, int64_t n) { GSTRIDE(i, n) a[i] = v; }

// out entries q: minor = minorOf[perm[q]], val = valIn[perm[q]]
__global__ void k_gather_entries(const int32_t* __restrict__ perm, const int32_t* __restrict__ minorIn,
                                 const double* __restrict__ valIn, int64_t nnz, int32_t* minorOut, double* valOut) {
  GSTRIDE(q, nnz) {
    const int p = perm[q];
    minorOut[q] = minorIn[p];
    valOut[q] = valIn[p];
  }
}
// beg[i] = first q with sortedMajor[q] >= i  (i = 0..nMajor)
__global__ void k_lower_bounds(const int32_t* __restrict__ sortedKeys, int64_t nnz, int64_t nQueries, int32_t* out) {
  GSTRIDE(i, nQueries) {
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((int64_t)(uint32_t)sortedKeys[mid] < i) lo = mid + 1; else hi = mid;
    }
    out[i] = (int32_t)lo;
  }
}

// ---- scaling --------------------------------------------------------------------
// one thread per major: max |a| (Ruiz) or left-to-right sum |a| (Pock-Chambolle, alpha = 1)
template <bool SUM>
__global__ void k_major_reduce(const int32_t* __restrict__ beg, const double* __restrict__ val, int nMajor,
                               double* out) {
  GSTRIDE(r, nMajor) {
    double s = 0.0;
    for (int p = beg[r]; p < beg[r + 1]; ++p) {
      const double a = fabs(val[p]);
      if (SUM) s += a;
      else if (a > s) s = a;
    }
    out[r] = (s == 0.0) ? 1.0 : sqrt(s);  // sqrt(max) / sqrt(sum^(1/1)); empty or zero majors -> 1
  }
}
// qdiag (QP, may be null): x = x'/cs  =>  1/2 q x^2 = 1/2 (q / cs^2) x'^2, two divisions per pass as applyScaling does
__global__ void k_apply_cols(const double* __restrict__ cs, int n, double* cost, double* lower, double* upper,
                             double* colScale, double* qdiag) {
  GSTRIDE(j, n) {
    cost[j] /= cs[j];
    lower[j] *= cs[j];
    upper[j] *= cs[j];
    colScale[j] *= cs[j];
    if (qdiag) qdiag[j] = (qdiag[j] / cs[j]) / cs[j];
  }
}
__global__ void k_apply_rows(const double* __restrict__ rs, int m, double* rhs, double* rowScale) {
  GSTRIDE(i, m) {
    rhs[i] /= rs[i];
    rowScale[i] *= rs[i];
  }
}
// a = (a / rs[row]) / cs[col], the operation order of scale_problem (cupdlp_scaling.c:17-45)
__global__ void k_scale_vals(const int32_t* __restrict__ rowOf, const int32_t* __restrict__ colOf,
                             const double* __restrict__ rs, const double* __restrict__ cs, int64_t nnz, double* val) {
  GSTRIDE(p, nnz) val[p] = (val[p] / rs[rowOf[p]]) / cs[colOf[p]];
}
// the off-diagonal part N of a QP's Hessian, one thread per slot: v = (v / cs[row]) / cs[col], the two divisions of
// applyScaling (pdlp_host.cpp) in its order; both factors are loaded before the first division
__global__ void k_scale_qoff(const int32_t* __restrict__ rowOf, const int32_t* __restrict__ colOf,
                             const double* __restrict__ cs, int64_t count, double* val) {
  GSTRIDE(p, count) {
    const double v = val[p];
    const double fr = cs[rowOf[p]], fc = cs[colOf[p]];
    val[p] = (v / fr) / fc;
  }
}
// HiPDLP (scaling.cc): MODE 0 sqrt(max|a|) (Ruiz), 1 sqrt(sum|a|) (Pock-Chambolle, alpha 1), 2 sqrt(sqrt(sum a^2)) (L2);
// zero or empty majors -> 1
template <int MODE>
__global__ void k_major_reduce_h(const int32_t* __restrict__ beg, const double* __restrict__ val, int nMajor,
                                 double* out) {
  GSTRIDE(r, nMajor) {
    double s = 0.0;
    for (int p = beg[r]; p < beg[r + 1]; ++p) {
      const double a = fabs(val[p]);
      if (MODE == 0) s = a > s ? a : s;
      else if (MODE == 1) s += a;
      else s += val[p] * val[p];
    }
    if (MODE == 0) out[r] = (s == 0.0) ? 1.0 : sqrt(s);
    else if (MODE == 1) out[r] = s > 0.0 ? sqrt(s) : 1.0;
    else out[r] = s > 0.0 ? sqrt(sqrt(s)) : 1.0;
  }
}
__global__ void k_apply_rows_h(const double* __restrict__ rs, int m, double* rowLower, double* rowUpper,
                               double* rowScale) {
  GSTRIDE(i, m) {
    if (rowLower[i] > -INFINITY) rowLower[i] /= rs[i];
    if (rowUpper[i] < INFINITY) rowUpper[i] /= rs[i];
    rowScale[i] *= rs[i];
  }
}
__global__ void k_apply_cols_h(const double* __restrict__ cs, int n, double* cost, double* lower, double* upper,
                               double* colScale) {
  GSTRIDE(j, n) {
    cost[j] /= cs[j];
    if (lower[j] > -INFINITY) lower[j] *= cs[j];
    if (upper[j] < INFINITY) upper[j] *= cs[j];
    colScale[j] *= cs[j];
  }
}
// a /= (rs[row] * cs[col]): Scaling::applyScaling, scaling.cc:251-259
__global__ void k_scale_vals_h(const int32_t* __restrict__ rowOf, const int32_t* __restrict__ colOf,
                               const double* __restrict__ rs, const double* __restrict__ cs, int64_t nnz, double* val) {
  GSTRIDE(p, nnz) val[p] /= (rs[rowOf[p]] * cs[colOf[p]]);
}
__global__ void k_is_eq(const int32_t* __restrict__ kind, const int32_t* __restrict__ rowNewIdx, int m, uint8_t* isEq) {
  GSTRIDE(i, m) isEq[rowNewIdx[i]] = isEqKind(kind[i]) ? 1 : 0;
}
__global__ void k_absmax_partial(const double* __restrict__ val, int64_t nnz, double* partial) {
  __shared__ double sm[kT];
  double mx = 0.0;
  GSTRIDE(p, nnz) { const double a = fabs(val[p]); if (a > mx) mx = a; }
  sm[threadIdx.x] = mx;
  __syncthreads();
  for (int s = kT / 2; s > 0; s >>= 1) {
    if (threadIdx.x < s && sm[threadIdx.x + s] > sm[threadIdx.x]) sm[threadIdx.x] = sm[threadIdx.x + s];
    __syncthreads();
  }
  if (threadIdx.x == 0) partial[blockIdx.x] = sm[0];
}

// ---- slab layout ------------------------------------------------------------------
// waveOf[r] = the wave that owns major r (waveBeg: first major of every wave, ascending; empty waves repeat a value)
__global__ void k_wave_of(const int32_t* __restrict__ waveBeg, int nWaves, int nMajor, int32_t* waveOf) {
  GSTRIDE(r, nMajor) {
    int lo = 0, hi = nWaves;  // last w with waveBeg[w] <= r
    while (hi - lo > 1) {
      const int mid = (lo + hi) >> 1;
      if (waveBeg[mid] <= (int)r) lo = mid; else hi = mid;
    }
    waveOf[r] = lo;
  }
}
__global__ void k_slab_keys(const int32_t* __restrict__ beg, const int32_t* __restrict__ major,
                            const int32_t* __restrict__ idx, int64_t nnz, const int32_t* __restrict__ waveOf, int S, int W,
                            int longLimit, uint32_t keyMax, uint32_t* keys) {
  GSTRIDE(p, nnz) {
    const int r = major[p];
    const int len = beg[r + 1] - beg[r];
    keys[p] = len > longLimit ? keyMax : (uint32_t)waveOf[r] * (uint32_t)S + ((uint32_t)idx[p] >> W);
  }
}
__global__ void k_slab_entries(const int32_t* __restrict__ perm, const int32_t* __restrict__ major,
                               const int32_t* __restrict__ idx, const double* __restrict__ valIn, int64_t nShort,
                               const int32_t* __restrict__ waveOf, const int32_t* __restrict__ waveBeg, int minorBits,
                               uint32_t* ent, double* val) {
  GSTRIDE(q, nShort) {
    const int p = perm[q];
    const int r = major[p];
    ent[q] = ((uint32_t)(r - waveBeg[waveOf[r]]) << minorBits) | (uint32_t)idx[p];
    val[q] = valIn[p];
  }
}
// wavePtr[w] = first q with sortedKey[q] >= w*S  (w = 0..nWaves; keyMax sorts after every wave)
__global__ void k_wave_ptr(const uint32_t* __restrict__ sortedKeys, int64_t nnz, int nWaves, int S, int32_t* out) {
  GSTRIDE(w, nWaves + 1) {
    const uint64_t key = (uint64_t)w * (uint64_t)S;
    int64_t lo = 0, hi = nnz;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      if ((uint64_t)sortedKeys[mid] < key) lo = mid + 1; else hi = mid;
    }
    out[w] = (int32_t)lo;
  }
}
__global__ void k_long_mask(const int32_t* __restrict__ beg, int nMajor, int longLimit, int nWords,
                            uint32_t* mask, int32_t* longFlag) {
  GSTRIDE(w, nWords) {  // bit r of the mask: major r is a long one
    uint32_t bits = 0;
    for (int k = 0; k < 32; ++k) {
      const int64_t r = w * 32 + k;
      if (r < nMajor && beg[r + 1] - beg[r] > longLimit) bits |= 1u << k;
    }
    mask[w] = bits;
  }
  GSTRIDE(r, nMajor) longFlag[r] = (beg[r + 1] - beg[r] > longLimit) ? 1 : 0;
}
// long-major compaction
__global__ void k_long_rows(const int32_t* __restrict__ beg, const int32_t* __restrict__ longFlag,
                            const int32_t* __restrict__ longRank, int nMajor, int32_t* longMap, int32_t* longLen) {
  GSTRIDE(r, nMajor) if (longFlag[r]) { longMap[longRank[r]] = (int)r; longLen[longRank[r]] = beg[r + 1] - beg[r]; }
}
__global__ void k_long_copy(const int32_t* __restrict__ beg, const int32_t* __restrict__ idx,
                            const double* __restrict__ val, const int32_t* __restrict__ longMap,
                            const int32_t* __restrict__ longBeg, int32_t* idxOut, double* valOut) {
  const int c = blockIdx.x;  // one block per long major
  const int r = longMap[c];
  const int src = beg[r], len = beg[r + 1] - beg[r], dst = longBeg[c];
  for (int k = threadIdx.x; k < len; k += blockDim.x) { idxOut[dst + k] = idx[src + k]; valOut[dst + k] = val[src + k]; }
}

// ---- the Hessian's extraction (gpuExtractHessian) ------------------------------------------------------------------------
// Integer work throughout: one thread per slot, entry or column, grid-stride, unit-stride loads of the caller's arrays;
// every scatter goes to a rank that a scan of 0/1 flags gave, so no two threads share a destination.
enum : unsigned long long { kHessSlotOutOfRange = 1, kHessSlotAbove = 2 };  // what is wrong with an offending slot

// col[p] = the column of slot p, as k_col_entries writes cscCol from a_start (q_start runs from 0 to nq without decreasing)
__global__ void k_hess_cols(const int32_t* __restrict__ qStart, int qDim, int32_t* col) {
  GSTRIDE(j, qDim)
    for (int p = qStart[j]; p < qStart[j + 1]; ++p) col[p] = (int)j;
}
// The host walk's tests in its order (extractHessian / extractHessianPattern): index outside [0, qDim); a zero value is not
// taken unless every slot is kept (== 0.0: -0.0 is dropped, a NaN is kept); diagonal; above the diagonal.  The smallest
// offending slot wins, as the walk meets it first: (p << 2) | kind, an integer minimum.
__global__ void k_hess_classify(const int32_t* __restrict__ qIndex, const double* __restrict__ qValue,
                                const int32_t* __restrict__ col, int64_t nq, int qDim, int keepAll, int32_t* diagFlag,
                                int32_t* offFlag, unsigned long long* offender) {
  GSTRIDE(p, nq) {
    const int i = qIndex[p], j = col[p];
    int d = 0, o = 0;
    if (i < 0 || i >= qDim) atomicMin(offender, ((unsigned long long)p << 2) | kHessSlotOutOfRange);
    else if (!keepAll && qValue[p] == 0.0) {}
    else if (i == j) d = 1;
    else if (i < j) atomicMin(offender, ((unsigned long long)p << 2) | kHessSlotAbove);
    else o = 1;
    diagFlag[p] = d;
    offFlag[p] = o;
  }
}
// the diagonal's sources in caller order; its starts follow from the ranks, since slots come column by column:
// dstBeg[j] = diagonal slots in front of column j (columns behind q_dim, slack columns included, have none)
__global__ void k_hess_diag_sources(const int32_t* __restrict__ diagFlag, const int32_t* __restrict__ diagRank, int64_t nq,
                                    int32_t* srcSlot) {
  GSTRIDE(p, nq) if (diagFlag[p]) srcSlot[diagRank[p]] = (int32_t)p;
}
__global__ void k_hess_diag_starts(const int32_t* __restrict__ qStart, const int32_t* __restrict__ diagRank, int qDim,
                                   int n, int32_t* dstBeg) {
  GSTRIDE(j, (int64_t)n + 1) dstBeg[j] = diagRank[qStart[j < qDim ? j : qDim]];
}
// taken off-diagonal slot p = (i, j), rank e of k: head entry e = (row i, column j), tail entry k + e = (row j, column i)
__global__ void k_hess_entries(const int32_t* __restrict__ qIndex, const int32_t* __restrict__ col,
                               const int32_t* __restrict__ offFlag, const int32_t* __restrict__ offRank, int64_t nq,
                               int64_t k, uint32_t* entCol, uint32_t* entRow, int32_t* entSrc) {
  GSTRIDE(p, nq) if (offFlag[p]) {
    const int64_t e = offRank[p];
    const uint32_t i = (uint32_t)qIndex[p], j = (uint32_t)col[p];
    entCol[e] = j; entRow[e] = i; entSrc[e] = (int32_t)p;
    entCol[k + e] = i; entRow[k + e] = j; entSrc[k + e] = (int32_t)p;
  }
}
__global__ void k_hess_permute(const int32_t* __restrict__ perm, const uint32_t* __restrict__ in, int64_t count, uint32_t* out) {
  GSTRIDE(q, count) out[q] = in[perm[q]];
}
// after both sorts entry q has row rowS[q], column colS[byRow[q]]: a run of equal (row, column) is one slot of N
__global__ void k_hess_run_heads(const uint32_t* __restrict__ rowS, const uint32_t* __restrict__ colS,
                                 const int32_t* __restrict__ byRow, int64_t count, int32_t* head) {
  GSTRIDE(q, count) head[q] = (q == 0 || rowS[q] != rowS[q - 1] || colS[byRow[q]] != colS[byRow[q - 1]]) ? 1 : 0;
}
// the off-diagonal destinations: entry q's source behind the diagonal's dcnt, and per run head slot d of N — its row, its
// column, its first source; the last entry closes the last run
__global__ void k_hess_finish(const uint32_t* __restrict__ rowS, const uint32_t* __restrict__ colS,
                              const int32_t* __restrict__ byRow, const int32_t* __restrict__ byCol,
                              const int32_t* __restrict__ entSrc, const int32_t* __restrict__ head,
                              const int32_t* __restrict__ headRank, int64_t count, int n, int32_t dcnt, int32_t* srcSlot,
                              int32_t* dstBeg, int32_t* offRow, int32_t* offCol) {
  GSTRIDE(q, count) {
    const int b = byRow[q];
    srcSlot[dcnt + q] = entSrc[byCol[b]];
    const int d = headRank[q];
    if (head[q]) {
      offRow[d] = (int32_t)rowS[q];
      offCol[d] = (int32_t)colS[b];
      dstBeg[n + d] = (int32_t)(dcnt + q);
    }
    if (q == count - 1) dstBeg[n + d + head[q]] = (int32_t)(dcnt + count);
  }
}

// ---- rocPRIM helpers -----------------------------------------------------------------
void exclusiveSum(const int32_t* in, int32_t* out, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  size_t bytes = 0;
  PDLP_HIP(rocprim::exclusive_scan(nullptr, bytes, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), s));
  DeviceArray<char> tmp;
  tmp.alloc(bytes);
  PDLP_HIP(rocprim::exclusive_scan(tmp.get(), bytes, in, out, (int32_t)0, (size_t)n, rocprim::plus<int32_t>(), s));
  PDLP_HIP(hipStreamSynchronize(s));
}
int bitsFor(uint64_t maxKey) {
  int b = 1;
  while (b < 32 && (maxKey >> b) != 0) ++b;
  return b;
}
// stable sort of (key, position) pairs; returns sorted keys and the permutation
void sortByKey(const uint32_t* keysIn, int64_t n, uint64_t maxKey, DeviceArray<uint32_t>& keysOut,
               DeviceArray<int32_t>& perm, hipStream_t s, size_t* scratchBytes = nullptr /* what it held besides its results */) {
  if (scratchBytes) *scratchBytes = 0;
  keysOut.alloc((size_t)n);
  perm.alloc((size_t)n);
  if (n <= 0) return;
  DeviceArray<int32_t> iota;
  iota.alloc((size_t)n);
  hipLaunchKernelGGL(k_iota, dim3(gridFor(n)), dim3(kT), 0, s, iota.get(), n);
  size_t bytes = 0;
  const unsigned endBit = (unsigned)bitsFor(maxKey);
  PDLP_HIP(rocprim::radix_sort_pairs(nullptr, bytes, keysIn, keysOut.get(), iota.get(), perm.get(), (size_t)n, 0u,
                                     endBit, s));
  DeviceArray<char> tmp;
  tmp.alloc(bytes);
  if (scratchBytes) *scratchBytes = bytes + sizeof(int32_t) * (size_t)n;
  PDLP_HIP(rocprim::radix_sort_pairs(tmp.get(), bytes, keysIn, keysOut.get(), iota.get(), perm.get(), (size_t)n, 0u,
                                     endBit, s));
  PDLP_HIP(hipStreamSynchronize(s));
}

template <typename T>
T fetchOne(const T* dev, hipStream_t s) {
  T v;
  PDLP_HIP(hipMemcpyAsync(&v, dev, sizeof(T), hipMemcpyDeviceToHost, s));
  PDLP_HIP(hipStreamSynchronize(s));
  return v;
}

// CSR <-> CSC by a stable sort on the minor index: the output majors keep their
// entries in ascending input-major order (what cupdlp_dcs_transpose produces).
void transposeOnDevice(const int32_t* majorIn, const int32_t* minorIn, const double* valIn, int64_t nnz,
                       int32_t nMajorOut, int32_t nMinorOut, hipStream_t s, DeviceCsrData& out,
                       DeviceArray<int32_t>* permOut = nullptr /* out slot -> in slot, for those who keep it */) {
  out.nMajor = nMajorOut;
  out.nMinor = nMinorOut;
  out.nnz = nnz;
  DeviceArray<uint32_t> keys;
  DeviceArray<int32_t> perm;
  sortByKey(reinterpret_cast<const uint32_t*>(minorIn), nnz, (uint64_t)std::max(nMajorOut, 1), keys, perm, s);
  out.major.alloc((size_t)nnz);
  out.idx.alloc((size_t)nnz + 1);
  out.val.alloc((size_t)nnz + 1);
  out.idx.zero(s);
  out.val.zero(s);
  out.beg.alloc((size_t)nMajorOut + 1);
  if (nnz > 0) {
    PDLP_HIP(hipMemcpyAsync(out.major.get(), keys.get(), sizeof(int32_t) * nnz, hipMemcpyDeviceToDevice, s));
    hipLaunchKernelGGL(k_gather_entries, dim3(gridFor(nnz)), dim3(kT), 0, s, perm.get(), majorIn, valIn, nnz,
                       out.idx.get(), out.val.get());
  }
  hipLaunchKernelGGL(k_lower_bounds, dim3(gridFor(nMajorOut + 1)), dim3(kT), 0, s,
                     reinterpret_cast<const int32_t*>(keys.get()), nnz, (int64_t)nMajorOut + 1, out.beg.get());
  PDLP_HIP(hipStreamSynchronize(s));
  if (permOut) *permOut = std::move(perm);
}

template <typename T>
void copyOf(DeviceArray<T>& dst, const DeviceArray<T>& src, hipStream_t s) {
  dst.alloc(src.size());
  if (src.size()) PDLP_HIP(hipMemcpyAsync(dst.get(), src.get(), sizeof(T) * src.size(), hipMemcpyDeviceToDevice, s));
}

}  // namespace

int32_t hessianExtractionReason(bool gpuSetup, bool sharded, bool hipdlp, bool switchOn, int32_t qDim, const int32_t* qStart) {
  if (!gpuSetup) return kHessHostSetup;
  if (sharded) return kHessSharded;
  if (hipdlp) return kHessHipdlp;
  if (qDim <= 0 || !qStart) return kHessNoSlots;
  if (qStart[0] != 0) return kHessStarts;
  for (int32_t j = 0; j < qDim; ++j)
    if (qStart[j + 1] < qStart[j]) return kHessStarts;
  if (qStart[qDim] <= 0) return kHessNoSlots;
  return switchOn ? kHessOnDevice : kHessSwitchOff;
}

// The map is built as the host walk builds it, by sorting instead of walking (tests/test_hessian_extraction_host.py
// holds the two against each other): all head entries in slot order, then all tail entries, sorted stably by column and
// then stably by row, are the walk's (row, column, source) sequence — a row's heads have columns below it, ascending with
// the slots; its tails columns above it, which the walk's insertion sort orders stably — and runs of equal (row, column)
// come in the order the walk adds repeated pairs.  k_hessian_validate / k_hessian_assemble (pdlp_update.hip) then do on the map what
// firstNegativeDiagonal / assembleHessian do, operation for operation — and extractHessian does the same ones on the taken
// slots: a source times the sense, the diagonal summed from 0.0, a slot of N from its first source.
void gpuExtractHessian(const pdlp_problem_t& P, int32_t n, hipStream_t s, DeviceProblem& D) {
  const auto t0 = std::chrono::steady_clock::now();
  const int32_t qDim = P.q_dim;
  const int64_t nq = P.q_start[qDim];
  // 1. the caller's arrays: 16 bytes per slot, 4 per column
  DeviceHessianInputs in;
  in.ownStart.alloc((size_t)qDim + 1); in.ownIndex.alloc((size_t)nq); in.ownValue.alloc((size_t)nq);
  in.ownStart.upload(P.q_start, (size_t)qDim + 1, s); in.ownIndex.upload(P.q_index, (size_t)nq, s); in.ownValue.upload(P.q_value, (size_t)nq, s);
  PDLP_HIP(hipStreamSynchronize(s));
  in.qStart = in.ownStart.get(); in.qIndex = in.ownIndex.get(); in.qValue = in.ownValue.get();
  D.secUploadHessian = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  gpuExtractHessianFromDevice(P, in, n, s, D);
}

// P: q_dim and a host copy of q_start; the slots are read from `in` alone
void gpuExtractHessianFromDevice(const pdlp_problem_t& P, DeviceHessianInputs& in, int32_t n, hipStream_t s, DeviceProblem& D) {
  const auto t1 = std::chrono::steady_clock::now();
  const int32_t qDim = P.q_dim;
  const int64_t nq = P.q_start[qDim];
  const bool keepAll = D.keepHessianPattern;
  size_t held = 0, peak = 0;  // HBM of the temporaries (not of what stays: qdiag, N, the kept map)
  auto got = [&](const auto& a) { held += sizeof(*a.get()) * a.size(); peak = std::max(peak, held); };
  auto rid = [&](auto& a) { held -= sizeof(*a.get()) * a.size(); a.release(); };
  // (the uploaded copies are temporaries of the extraction; a caller's own arrays in HBM are not, and count as nothing)
  got(in.ownStart); got(in.ownIndex); got(in.ownValue);
  const int32_t* const qStartDev = in.qStart;
  const int32_t* const qIndexDev = in.qIndex;
  const double* const qValueDev = in.qValue;

  // 2. classify; flags and ranks have one element behind the last slot, so that a scan ends in its total
  DeviceArray<int32_t> col, diagFlag, offFlag, diagRank, offRank;
  DeviceArray<unsigned long long> offender;
  col.alloc((size_t)nq); diagFlag.alloc((size_t)nq + 1); offFlag.alloc((size_t)nq + 1);
  diagRank.alloc((size_t)nq + 1); offRank.alloc((size_t)nq + 1); offender.alloc(1);
  got(col); got(diagFlag); got(offFlag); got(diagRank); got(offRank);
  diagFlag.zero(s);
  offFlag.zero(s);
  PDLP_HIP(hipMemsetAsync(offender.get(), 0xff, sizeof(unsigned long long), s));
  hipLaunchKernelGGL(k_hess_cols, dim3(gridFor(qDim)), dim3(kT), 0, s, qStartDev, qDim, col.get());
  hipLaunchKernelGGL(k_hess_classify, dim3(gridFor(nq)), dim3(kT), 0, s, qIndexDev, qValueDev, col.get(), nq, qDim,
                     keepAll ? 1 : 0, diagFlag.get(), offFlag.get(), offender.get());
  PDLP_HIP(hipGetLastError());
  const unsigned long long first = fetchOne(offender.get(), s);
  if (first != ~0ull) {  // the walk's sentences (pdlp_host.cpp), for the slot it would have met first
    const int64_t p = (int64_t)(first >> 2);
    if ((first & 3) == kHessSlotOutOfRange) throw std::runtime_error("Hessian index out of range");
    const int32_t j = fetchOne(col.get() + p, s);
    throw std::runtime_error("pdlp_mi355x: the Hessian must be given by its lower triangle (entry (" + std::to_string(fetchOne(qIndexDev + p, s)) +
                             "," + std::to_string(j) + ") lies above the diagonal)");
  }

  // 3. counts, compaction, the two sorts
  exclusiveSum(diagFlag.get(), diagRank.get(), nq + 1, s);
  exclusiveSum(offFlag.get(), offRank.get(), nq + 1, s);
  const int64_t dcnt = fetchOne(diagRank.get() + nq, s), k = fetchOne(offRank.get() + nq, s), nEnt = 2 * k;
  D.hessianTaken = dcnt + k;
  D.hessianOffSlots = 0;
  auto done = [&] {
    PDLP_HIP(hipStreamSynchronize(s));
    D.hessianTempBytes = (int64_t)peak;
    D.secExtract = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
  };
  if (!keepAll && dcnt + k == 0) return done();  // every value is zero: an LP
  if (nEnt > 0x7fffffff || dcnt + nEnt > 0x7fffffff) throw std::runtime_error("Hessian too large");
  DeviceArray<int32_t> dstBeg, srcSlot;
  srcSlot.alloc((size_t)std::max<int64_t>(dcnt + nEnt, 1));
  if (!keepAll) got(srcSlot);  // (a plain solver's map is a temporary too)
  hipLaunchKernelGGL(k_hess_diag_sources, dim3(gridFor(nq)), dim3(kT), 0, s, diagFlag.get(), diagRank.get(), nq, srcSlot.get());
  DeviceArray<uint32_t> colS, rowS;     // every entry's column after the first sort, its row after the second
  DeviceArray<int32_t> byCol, byRow, entSrc;  // the two permutations, every entry's source slot
  DeviceArray<int32_t> head, headRank;
  int32_t nOff = 0;
  if (k > 0) {
    DeviceArray<uint32_t> entCol, entRow, rowIn;
    entCol.alloc((size_t)nEnt); entRow.alloc((size_t)nEnt); entSrc.alloc((size_t)nEnt);
    got(entCol); got(entRow); got(entSrc);
    hipLaunchKernelGGL(k_hess_entries, dim3(gridFor(nq)), dim3(kT), 0, s, qIndexDev, col.get(), offFlag.get(), offRank.get(), nq, k,
                       entCol.get(), entRow.get(), entSrc.get());
    PDLP_HIP(hipStreamSynchronize(s));
    rid(col); rid(diagFlag); rid(offFlag); rid(offRank); rid(in.ownIndex);
    size_t scratch = 0;
    sortByKey(entCol.get(), nEnt, (uint64_t)qDim, colS, byCol, s, &scratch);
    peak = std::max(peak, held + scratch + 2 * sizeof(int32_t) * (size_t)nEnt);
    got(colS); got(byCol);
    rid(entCol);
    rowIn.alloc((size_t)nEnt);
    got(rowIn);
    hipLaunchKernelGGL(k_hess_permute, dim3(gridFor(nEnt)), dim3(kT), 0, s, byCol.get(), entRow.get(), nEnt, rowIn.get());
    PDLP_HIP(hipStreamSynchronize(s));
    rid(entRow);
    sortByKey(rowIn.get(), nEnt, (uint64_t)qDim, rowS, byRow, s, &scratch);
    peak = std::max(peak, held + scratch + 2 * sizeof(int32_t) * (size_t)nEnt);
    got(rowS); got(byRow);
    rid(rowIn);
    // 4. runs of equal (row, column) -> the slots of N
    head.alloc((size_t)nEnt + 1); headRank.alloc((size_t)nEnt + 1);
    got(head); got(headRank);
    head.zero(s);
    hipLaunchKernelGGL(k_hess_run_heads, dim3(gridFor(nEnt)), dim3(kT), 0, s, rowS.get(), colS.get(), byRow.get(), nEnt, head.get());
    exclusiveSum(head.get(), headRank.get(), nEnt + 1, s);
    nOff = fetchOne(headRank.get() + nEnt, s);
  }
  dstBeg.alloc((size_t)n + (size_t)nOff + 1);
  if (!keepAll) got(dstBeg);
  hipLaunchKernelGGL(k_hess_diag_starts, dim3(gridFor((int64_t)n + 1)), dim3(kT), 0, s, qStartDev, diagRank.get(), qDim, n, dstBeg.get());
  if (nOff > 0) {
    D.N.nMajor = D.N.nMinor = n;
    D.N.nnz = nOff;
    D.N.beg.alloc((size_t)n + 1);
    D.N.idx.alloc((size_t)nOff + 1);  // one pad element: the kernels clamp, never predicate, their loads
    D.N.val.alloc((size_t)nOff + 1);
    D.N.major.alloc((size_t)nOff);
    D.N.idx.zero(s);
    D.N.val.zero(s);
    hipLaunchKernelGGL(k_hess_finish, dim3(gridFor(nEnt)), dim3(kT), 0, s, rowS.get(), colS.get(), byRow.get(), byCol.get(), entSrc.get(),
                       head.get(), headRank.get(), nEnt, n, (int32_t)dcnt, srcSlot.get(), dstBeg.get(), D.N.major.get(), D.N.idx.get());
    hipLaunchKernelGGL(k_lower_bounds, dim3(gridFor((int64_t)n + 1)), dim3(kT), 0, s, D.N.major.get(), (int64_t)nOff, (int64_t)n + 1,
                       D.N.beg.get());
  }
  PDLP_HIP(hipGetLastError());
  D.hessianOffSlots = nOff;

  // 5. the diagonal's sign, then the values
  DeviceArray<int32_t> bad;
  bad.alloc(1);
  PDLP_HIP(hipMemcpyAsync(bad.get(), &n, sizeof(int32_t), hipMemcpyHostToDevice, s));
  launchHessianValidate(dstBeg.get(), srcSlot.get(), qValueDev, D.sense, n, bad.get(), s);
  if (fetchOne(bad.get(), s) < n)
    throw std::runtime_error("pdlp_mi355x: the Hessian is not positive semidefinite for this objective sense");
  D.qdiag.alloc((size_t)n);
  launchHessianAssemble(dstBeg.get(), srcSlot.get(), qValueDev, D.sense, n, nOff, D.qdiag.get(), nOff > 0 ? D.N.val.get() : nullptr, s);
  if (keepAll) {  // the map and the unscaled Hessian stay, sized as Solver::keepHessian sizes its uploads
    DeviceHessianMap& K = D.kmap;
    K.nSlots = (int32_t)nq;
    K.nOff = nOff;
    K.dstBeg = std::move(dstBeg);
    K.srcSlot = std::move(srcSlot);
    K.offRow.alloc((size_t)std::max(nOff, 1)); K.offCol.alloc((size_t)std::max(nOff, 1));
    if (nOff > 0) {
      PDLP_HIP(hipMemcpyAsync(K.offRow.get(), D.N.major.get(), sizeof(int32_t) * (size_t)nOff, hipMemcpyDeviceToDevice, s));
      PDLP_HIP(hipMemcpyAsync(K.offCol.get(), D.N.idx.get(), sizeof(int32_t) * (size_t)nOff, hipMemcpyDeviceToDevice, s));
      K.qoff0.alloc((size_t)nOff);
      PDLP_HIP(hipMemcpyAsync(K.qoff0.get(), D.N.val.get(), sizeof(double) * (size_t)nOff, hipMemcpyDeviceToDevice, s));
    }
    if (!D.keepMatrix) {  // (else MatrixKeep::qdiag0 holds it)
      K.qdiag0.alloc((size_t)n);
      PDLP_HIP(hipMemcpyAsync(K.qdiag0.get(), D.qdiag.get(), sizeof(double) * (size_t)n, hipMemcpyDeviceToDevice, s));
    }
  }
  done();  // 6. the temporaries go out of scope here, before any layout is built
}

void gpuFormulateValues(const int32_t* aStart, const int32_t* aIndex, const double* aValue, const int32_t* rowKind,
                        const int32_t* rowNewIdx, int32_t n0, int32_t m, int64_t nnz0, int64_t nSlack, double* cscVal,
                        hipStream_t s) {
  hipLaunchKernelGGL(k_col_entries<true>, dim3(gridFor(n0)), dim3(kT), 0, s, aStart, aIndex, aValue, rowKind, rowNewIdx, n0, m,
                     (int32_t*)nullptr, (int32_t*)nullptr, cscVal, (int32_t*)nullptr);
  if (nSlack > 0) hipLaunchKernelGGL(k_fill_d, dim3(gridFor(nSlack)), dim3(kT), 0, s, cscVal + nnz0, -1.0, nSlack);
  PDLP_HIP(hipGetLastError());
}

void gpuFill(double* a, double v, int64_t count, hipStream_t s) {
  if (count > 0) hipLaunchKernelGGL(k_fill_d, dim3(gridFor(count)), dim3(kT), 0, s, a, v, count);
}

// Ruiz x10 in the infinity norm, then Pock-Chambolle alpha = 1 (cupdlp_scaling.c:47-231); both copies of the matrix
// (reference-order CSC for the column passes, CSR for the row passes) receive the same two divisions, so they stay
// bit-identical
int32_t gpuScalePasses(const ScaleOperands& o, hipStream_t s) {
  const int32_t n = o.n, m = o.m;
  const int64_t nnz = o.nnz;
  DeviceArray<double> cs, rs;
  cs.alloc(n);
  rs.alloc(m);
  int32_t nPass = 0;
  auto pass = [&](bool sum) {
    if (sum) {
      hipLaunchKernelGGL(k_major_reduce<true>, dim3(gridFor(n)), dim3(kT), 0, s, o.cscBeg, o.cscVal, n, cs.get());
      hipLaunchKernelGGL(k_major_reduce<true>, dim3(gridFor(m)), dim3(kT), 0, s, o.aBeg, o.aVal, m, rs.get());
    } else {
      hipLaunchKernelGGL(k_major_reduce<false>, dim3(gridFor(n)), dim3(kT), 0, s, o.cscBeg, o.cscVal, n, cs.get());
      hipLaunchKernelGGL(k_major_reduce<false>, dim3(gridFor(m)), dim3(kT), 0, s, o.aBeg, o.aVal, m, rs.get());
    }
    hipLaunchKernelGGL(k_apply_cols, dim3(gridFor(n)), dim3(kT), 0, s, cs.get(), n, o.cost, o.lower, o.upper, o.colScale, o.qdiag);
    if (o.qoffVal && o.qoffCount > 0)  // N follows the columns like qdiag; the factors come from the matrix alone
      hipLaunchKernelGGL(k_scale_qoff, dim3(gridFor(o.qoffCount)), dim3(kT), 0, s, o.qoffRow, o.qoffCol, cs.get(), o.qoffCount, o.qoffVal);
    hipLaunchKernelGGL(k_apply_rows, dim3(gridFor(m)), dim3(kT), 0, s, rs.get(), m, o.rhs, o.rowScale);
    hipLaunchKernelGGL(k_scale_vals, dim3(gridFor(nnz)), dim3(kT), 0, s, o.cscIdx, o.cscCol, rs.get(), cs.get(), nnz, o.cscVal);
    hipLaunchKernelGGL(k_scale_vals, dim3(gridFor(nnz)), dim3(kT), 0, s, o.aMajor, o.aIdx, rs.get(), cs.get(), nnz, o.aVal);
    if (o.csPass) {
      if (n > 0) PDLP_HIP(hipMemcpyAsync(o.csPass + (size_t)nPass * n, cs.get(), sizeof(double) * n, hipMemcpyDeviceToDevice, s));
      if (m > 0) PDLP_HIP(hipMemcpyAsync(o.rsPass + (size_t)nPass * m, rs.get(), sizeof(double) * m, hipMemcpyDeviceToDevice, s));
    }
    ++nPass;
  };
  for (int it = 0; it < 10; ++it) pass(false);
  pass(true);
  PDLP_HIP(hipStreamSynchronize(s));
  return nPass;
}

double gpuAbsMax(const double* val, int64_t count, hipStream_t s) {
  const int nb = 1024;
  DeviceArray<double> part;
  part.alloc(nb);
  hipLaunchKernelGGL(k_absmax_partial, dim3(nb), dim3(kT), 0, s, val, count, part.get());
  std::vector<double> h(nb);
  part.download(h.data(), nb, s);
  PDLP_HIP(hipStreamSynchronize(s));
  double mx = 0.0;
  for (double v : h) mx = std::max(mx, v);
  return mx;
}

void gpuPrepare(const pdlp_problem_t& P, bool doScale, hipStream_t s, DeviceProblem& D, const HipdlpSetup* hp) {
  validateProblem(P);
  const int32_t n0 = P.num_col, m = P.num_row;
  const int64_t nnz0 = n0 > 0 ? P.a_start[n0] : 0;
  if (nnz0 > 0 && (!P.a_index || !P.a_value)) throw std::runtime_error("null matrix arrays");
  for (int32_t j = 0; j < n0; ++j)
    if (P.a_start[j + 1] < P.a_start[j]) throw std::runtime_error("a_start not monotone");

  // upload the caller's arrays
  DeviceInputs in;
  DeviceArray<double> aValue, cIn, clIn, cuIn, rlIn, ruIn;
  in.ownStart.alloc((size_t)n0 + 1); in.ownIndex.alloc((size_t)nnz0); aValue.alloc((size_t)nnz0);
  cIn.alloc(n0); clIn.alloc(n0); cuIn.alloc(n0); rlIn.alloc(m); ruIn.alloc(m);
  in.ownStart.upload(P.a_start, (size_t)n0 + 1, s); in.ownIndex.upload(P.a_index, (size_t)nnz0, s);
  aValue.upload(P.a_value, (size_t)nnz0, s);
  cIn.upload(P.col_cost, n0, s); clIn.upload(P.col_lower, n0, s); cuIn.upload(P.col_upper, n0, s);
  rlIn.upload(P.row_lower, m, s); ruIn.upload(P.row_upper, m, s);
  in.aStart = in.ownStart.get(); in.aIndex = in.ownIndex.get(); in.aValue = aValue.get();
  in.colCost = cIn.get(); in.colLower = clIn.get(); in.colUpper = cuIn.get(); in.rowLower = rlIn.get(); in.rowUpper = ruIn.get();
  gpuPrepareFromDevice(P, in, doScale, s, D, hp);
}

// P: the sizes, the scalars and HOST copies of a_start, col_cost, row_lower, row_upper and q_start (the monotone checks,
// the left-to-right norms, the Hessian rule); every other array of P is only asked whether it is NULL.  The caller has
// made validateProblem's checks of the starts.
void gpuPrepareFromDevice(const pdlp_problem_t& P, DeviceInputs& in, bool doScale, hipStream_t s, DeviceProblem& D,
                          const HipdlpSetup* hp) {
  const bool H = hp != nullptr;  // HiPDLP form (pdhg.cc:152-357 + scaling.cc) instead of the cuPDLP-C one
  const int32_t n0 = P.num_col, m = P.num_row;
  const int64_t nnz0 = n0 > 0 ? P.a_start[n0] : 0;
  D.n0 = n0;
  D.m = m;
  D.offset = P.offset;
  D.sense = P.sense < 0 ? -1.0 : 1.0;
  const double costSense = H ? 1.0 : D.sense;  // HiPDLP does not apply the objective sense (pdhg.cc:171)

  // rows: classify, rank, permute
  DeviceArray<int32_t> kind, eqF, inF, slF, eqR, inR, slR, rowNew;
  kind.alloc(m); eqF.alloc(m); inF.alloc(m); slF.alloc(m); eqR.alloc(m); inR.alloc(m); slR.alloc(m); rowNew.alloc(m);
  hipLaunchKernelGGL(k_row_classify, dim3(gridFor(m)), dim3(kT), 0, s, in.rowLower, in.rowUpper, m,
                     H ? (double)INFINITY : kBoundInf, H ? (int)kRowFree : (int)kRowBound, kind.get(), eqF.get(),
                     inF.get(), slF.get());
  exclusiveSum(eqF.get(), eqR.get(), m, s);
  exclusiveSum(inF.get(), inR.get(), m, s);
  exclusiveSum(slF.get(), slR.get(), m, s);
  int32_t nEq = 0, nSlack = 0;
  if (m > 0) {
    nEq = fetchOne(eqR.get() + (m - 1), s) + fetchOne(eqF.get() + (m - 1), s);
    nSlack = fetchOne(slR.get() + (m - 1), s) + fetchOne(slF.get() + (m - 1), s);
  }
  if ((int64_t)n0 + nSlack > std::numeric_limits<int32_t>::max() ||
      nnz0 + nSlack > std::numeric_limits<int32_t>::max())
    throw std::runtime_error("problem exceeds 32-bit index range");
  const int32_t n = n0 + nSlack;
  const int64_t nnz = nnz0 + nSlack;
  D.n = n; D.nEqs = nEq; D.nnz = nnz;

  D.cost.alloc(n); D.lower.alloc(n); D.upper.alloc(n); D.rhs.alloc(m); D.colScale.alloc(n); D.rowScale.alloc(m);
  if (H) { D.rowUpper.alloc(m); D.rowIsEq.alloc((size_t)m); }
  DeviceArray<int32_t> cscBeg, cscIdx, cscCol, bad;
  DeviceArray<double> cscVal;
  cscBeg.alloc((size_t)n + 1); cscIdx.alloc((size_t)nnz); cscCol.alloc((size_t)nnz); cscVal.alloc((size_t)nnz);
  bad.alloc(1);
  bad.zero(s);
  hipLaunchKernelGGL(k_col_setup, dim3(gridFor(n0)), dim3(kT), 0, s, in.colCost, in.colLower, in.colUpper, in.aStart,
                     n0, costSense, H ? 0 : 1, D.cost.get(), D.lower.get(), D.upper.get(), cscBeg.get());
  hipLaunchKernelGGL(k_row_finish, dim3(gridFor(m)), dim3(kT), 0, s, in.rowLower, in.rowUpper, kind.get(), eqR.get(),
                     inR.get(), slR.get(), m, n0, nEq, nnz0, rowNew.get(), D.rhs.get(), D.cost.get(), D.lower.get(),
                     D.upper.get(), cscBeg.get(), cscIdx.get(), cscCol.get(), cscVal.get(),
                     H ? D.rowUpper.get() : nullptr);
  if (H) hipLaunchKernelGGL(k_is_eq, dim3(gridFor(m)), dim3(kT), 0, s, kind.get(), rowNew.get(), m, D.rowIsEq.get());
  {
    const int32_t last = (int32_t)nnz;
    PDLP_HIP(hipMemcpyAsync(cscBeg.get() + n, &last, sizeof(int32_t), hipMemcpyHostToDevice, s));
    PDLP_HIP(hipStreamSynchronize(s));
  }
  hipLaunchKernelGGL(k_col_entries<false>, dim3(gridFor(n0)), dim3(kT), 0, s, in.aStart, in.aIndex, in.aValue,
                     kind.get(), rowNew.get(), n0, m, cscIdx.get(), cscCol.get(), cscVal.get(), bad.get());
  if (fetchOne(bad.get(), s) != 0) throw std::runtime_error("row index out of range");

  // host copies of the row bookkeeping; norms of the UNSCALED formulated data, summed
  // left to right on the host exactly as Init_Scaling does (cupdlp_scaling.c:395-425)
  D.rowKind.resize(m);
  D.rowNewIdx.resize(m);
  kind.download(D.rowKind.data(), m, s);
  rowNew.download(D.rowNewIdx.data(), m, s);
  PDLP_HIP(hipStreamSynchronize(s));
  D.normCost = unscaledNormCost(P.col_cost, n0, costSense);
  D.normRhs = unscaledNormRhs(P.row_lower, P.row_upper, D.rowKind.data(), m);

  // A by rows (ascending column): stable sort of the column-major entries by row
  const bool keepM = D.keepMatrix && !H;
  transposeOnDevice(cscCol.get(), cscIdx.get(), cscVal.get(), nnz, m, n, s, D.A, keepM ? &D.keep.permA : nullptr);

  // scaling: Ruiz x10 in the infinity norm, then Pock-Chambolle alpha = 1 (cupdlp_scaling.c:47-231);
  // both copies of the matrix (reference-order CSC for the column passes, CSR for the row
  // passes) receive the same two divisions, so they stay bit-identical
  hipLaunchKernelGGL(k_fill_d, dim3(gridFor(n)), dim3(kT), 0, s, D.colScale.get(), 1.0, (int64_t)n);
  hipLaunchKernelGGL(k_fill_d, dim3(gridFor(m)), dim3(kT), 0, s, D.rowScale.get(), 1.0, (int64_t)m);
  if (H) {
    // HiPDLP: columns are kept with ascending row index (pdhg.cc:311), so the column passes run on A' and
    // both copies receive the identical division a /= (rs * cs) (scaling.cc:251-259)
    transposeOnDevice(D.A.major.get(), D.A.idx.get(), D.A.val.get(), nnz, n, m, s, D.At);
    if (doScale && (hp->ruiz || hp->pc || hp->l2)) {
      DeviceArray<double> cs, rs;
      cs.alloc(n);
      rs.alloc(m);
      auto pass = [&](int mode) {
        if (mode == 0) {
          hipLaunchKernelGGL(k_major_reduce_h<0>, dim3(gridFor(n)), dim3(kT), 0, s, D.At.beg.get(), D.At.val.get(), n, cs.get());
          hipLaunchKernelGGL(k_major_reduce_h<0>, dim3(gridFor(m)), dim3(kT), 0, s, D.A.beg.get(), D.A.val.get(), m, rs.get());
        } else if (mode == 1) {
          hipLaunchKernelGGL(k_major_reduce_h<1>, dim3(gridFor(n)), dim3(kT), 0, s, D.At.beg.get(), D.At.val.get(), n, cs.get());
          hipLaunchKernelGGL(k_major_reduce_h<1>, dim3(gridFor(m)), dim3(kT), 0, s, D.A.beg.get(), D.A.val.get(), m, rs.get());
        } else {
          hipLaunchKernelGGL(k_major_reduce_h<2>, dim3(gridFor(n)), dim3(kT), 0, s, D.At.beg.get(), D.At.val.get(), n, cs.get());
          hipLaunchKernelGGL(k_major_reduce_h<2>, dim3(gridFor(m)), dim3(kT), 0, s, D.A.beg.get(), D.A.val.get(), m, rs.get());
        }
        hipLaunchKernelGGL(k_apply_cols_h, dim3(gridFor(n)), dim3(kT), 0, s, cs.get(), n, D.cost.get(), D.lower.get(),
                           D.upper.get(), D.colScale.get());
        hipLaunchKernelGGL(k_apply_rows_h, dim3(gridFor(m)), dim3(kT), 0, s, rs.get(), m, D.rhs.get(),
                           D.rowUpper.get(), D.rowScale.get());
        // A: major = row, idx = column;  A': major = column, idx = row
        hipLaunchKernelGGL(k_scale_vals_h, dim3(gridFor(nnz)), dim3(kT), 0, s, D.A.major.get(), D.A.idx.get(), rs.get(),
                           cs.get(), nnz, D.A.val.get());
        hipLaunchKernelGGL(k_scale_vals_h, dim3(gridFor(nnz)), dim3(kT), 0, s, D.At.idx.get(), D.At.major.get(), rs.get(),
                           cs.get(), nnz, D.At.val.get());
      };
      if (hp->ruiz) for (int it = 0; it < hp->ruizIters; ++it) pass(0);
      if (hp->pc) pass(1);
      if (hp->l2) pass(2);
      D.scaled = true;
      PDLP_HIP(hipStreamSynchronize(s));
    }
    D.hColScale.resize(n);
    D.hRowScale.resize(m);
    D.colScale.download(D.hColScale.data(), n, s);
    D.rowScale.download(D.hRowScale.data(), m, s);
    PDLP_HIP(hipStreamSynchronize(s));
    return;
  }
  // QP (cuPDLP-C form): the diagonal of Q, with the objective sense, rides along with the column scaling, and so does
  // the off-diagonal part N.  The host walk (pdlp_host.cpp) is the one definition of N's entry order and of every
  // refusal; gpuExtractHessian restates it on the device where the rule allows, else the walk's result is uploaded with a
  // row index per slot.  The checks the walk makes before its first slot are made here, in its words, for both.
  D.hessianReason = hessianExtractionReason(true, D.hessianSharded, false, D.hessianSwitchOn, P.q_dim, P.q_start);
  if (D.hessianReason == kHessOnDevice) {
    if (P.q_dim > P.num_col) throw std::runtime_error("Hessian dimension exceeds the number of columns");
    if (!P.q_index || !P.q_value) throw std::runtime_error("null Hessian arrays");
    if (in.hessian) gpuExtractHessianFromDevice(P, *in.hessian, n, s, D);
    else gpuExtractHessian(P, n, s, D);
  } else {
    std::vector<double> q;
    Compressed off;
    const auto t0 = std::chrono::steady_clock::now();
    if (D.keepHessianPattern) extractHessianKept(P, D.sense, n, q, off, D.hmap);
    else extractHessian(P, D.sense, n, q, off);
    const auto t1 = std::chrono::steady_clock::now();
    D.secExtract = std::chrono::duration<double>(t1 - t0).count();
    if (!q.empty()) {
      D.qdiag.alloc((size_t)n);
      D.qdiag.upload(q.data(), (size_t)n, s);
    }
    std::vector<int32_t> offRow;
    if (!off.beg.empty()) {
      const size_t nOff = off.idx.size();
      offRow.resize(nOff);
      for (int32_t r = 0; r < n; ++r)
        for (int32_t p = off.beg[r]; p < off.beg[r + 1]; ++p) offRow[p] = r;
      D.N.nMajor = D.N.nMinor = n;
      D.N.nnz = (int64_t)nOff;
      D.N.beg.alloc((size_t)n + 1);
      D.N.idx.alloc(nOff + 1);  // one pad element: the kernels clamp, never predicate, their loads
      D.N.val.alloc(nOff + 1);
      D.N.major.alloc(std::max<size_t>(nOff, 1));
      D.N.idx.zero(s);
      D.N.val.zero(s);
      D.N.beg.upload(off.beg.data(), (size_t)n + 1, s);
      D.N.idx.upload(off.idx.data(), nOff, s);
      D.N.val.upload(off.val.data(), nOff, s);
      D.N.major.upload(offRow.data(), nOff, s);
    }
    PDLP_HIP(hipStreamSynchronize(s));  // q, off and offRow go out of scope
    D.secUploadHessian = std::chrono::duration<double>(std::chrono::steady_clock::now() - t1).count();
    D.hessianOffSlots = (int64_t)off.idx.size();
    if (D.keepHessianPattern && !q.empty()) {
      D.hQdiag0 = std::move(q);
      D.hQoff0 = std::move(off.val);
    }
  }
  if (keepM) {  // the unscaled formulated data: new matrix values change every factor, and un-scaling does not give these bits
    copyOf(D.keep.cost0, D.cost, s); copyOf(D.keep.lower0, D.lower, s); copyOf(D.keep.upper0, D.upper, s);
    copyOf(D.keep.rhs0, D.rhs, s);
    if (D.qdiag.size()) copyOf(D.keep.qdiag0, D.qdiag, s);
  }
  if (doScale) {
    constexpr int kPasses = 11;  // Ruiz x 10 + Pock-Chambolle
    if (D.keepPasses) { D.csPass.alloc((size_t)kPasses * n); D.rsPass.alloc((size_t)kPasses * m); }
    ScaleOperands o;
    o.n = n; o.m = m; o.nnz = nnz;
    o.cscBeg = cscBeg.get(); o.cscIdx = cscIdx.get(); o.cscCol = cscCol.get(); o.cscVal = cscVal.get();
    o.aBeg = D.A.beg.get(); o.aMajor = D.A.major.get(); o.aIdx = D.A.idx.get(); o.aVal = D.A.val.get();
    o.cost = D.cost.get(); o.lower = D.lower.get(); o.upper = D.upper.get(); o.rhs = D.rhs.get();
    o.colScale = D.colScale.get(); o.rowScale = D.rowScale.get();
    o.qdiag = D.qdiag.size() ? D.qdiag.get() : nullptr;
    if (D.N.nnz > 0) { o.qoffRow = D.N.major.get(); o.qoffCol = D.N.idx.get(); o.qoffVal = D.N.val.get(); o.qoffCount = D.N.nnz; }
    if (D.keepPasses) { o.csPass = D.csPass.get(); o.rsPass = D.rsPass.get(); }
    const auto tp = std::chrono::steady_clock::now();
    const int32_t done = gpuScalePasses(o, s);
    D.secPasses = std::chrono::duration<double>(std::chrono::steady_clock::now() - tp).count();
    if (D.keepPasses) D.nPass = done;
    D.scaled = true;
  }

  // max |a_ij| of the scaled matrix (initial step size, cupdlp_step.c:360-365)
  D.matNormInf = gpuAbsMax(cscVal.get(), nnz, s);

  // A' by columns with ascending row: stable sort of the row-major entries by column
  transposeOnDevice(D.A.major.get(), D.A.idx.get(), D.A.val.get(), nnz, n, m, s, D.At, keepM ? &D.keep.permAt : nullptr);
  if (keepM) {  // the arrays a plain set-up frees here; the layouts take D.A's, so the row-major structure is copied
    MatrixKeep& K = D.keep;
    K.nnz0 = nnz0;
    if (in.ownStart.size()) {
      K.aStart = std::move(in.ownStart); K.aIndex = std::move(in.ownIndex);
    } else {  // the caller's own arrays in HBM: copied, the caller may free them after the return
      K.aStart.alloc((size_t)n0 + 1); K.aIndex.alloc((size_t)nnz0);
      PDLP_HIP(hipMemcpyAsync(K.aStart.get(), in.aStart, sizeof(int32_t) * ((size_t)n0 + 1), hipMemcpyDeviceToDevice, s));
      if (nnz0 > 0) PDLP_HIP(hipMemcpyAsync(K.aIndex.get(), in.aIndex, sizeof(int32_t) * (size_t)nnz0, hipMemcpyDeviceToDevice, s));
    }
    K.cscBeg = std::move(cscBeg); K.cscIdx = std::move(cscIdx); K.cscCol = std::move(cscCol); K.cscVal = std::move(cscVal);
    copyOf(K.aBeg, D.A.beg, s); copyOf(K.aMajor, D.A.major, s);
    K.aIdx.alloc((size_t)nnz); K.aVal.alloc((size_t)nnz);
    if (nnz > 0) {
      PDLP_HIP(hipMemcpyAsync(K.aIdx.get(), D.A.idx.get(), sizeof(int32_t) * nnz, hipMemcpyDeviceToDevice, s));
      PDLP_HIP(hipMemcpyAsync(K.aVal.get(), D.A.val.get(), sizeof(double) * nnz, hipMemcpyDeviceToDevice, s));
    }
  }

  // host copies: scale vectors (postsolve / hot start) and the left-to-right sums of
  // the scaled c and b that PDHG_Init_Step_Sizes needs (cupdlp_step.c:349-358)
  D.hColScale.resize(n);
  D.hRowScale.resize(m);
  std::vector<double> hc(n), hb(m);
  D.colScale.download(D.hColScale.data(), n, s);
  D.rowScale.download(D.hRowScale.data(), m, s);
  D.cost.download(hc.data(), n, s);
  D.rhs.download(hb.data(), m, s);
  PDLP_HIP(hipStreamSynchronize(s));
  D.sumCost2 = 0.0;
  for (double v : hc) D.sumCost2 += v * v;
  D.sumRhs2 = 0.0;
  for (double v : hb) D.sumRhs2 += v * v;
}

// pdlp_host.cpp slabColdCounts on the device: how many majors touch every minor, then the cold entries of every major
__global__ void k_minor_count(const int32_t* __restrict__ idx, int64_t nnz, int32_t* count) {
  GSTRIDE(p, nnz) atomicAdd(count + idx[p], 1);
}
__global__ void k_major_cold(const int32_t* __restrict__ beg, const int32_t* __restrict__ idx, const int32_t* __restrict__ count,
                             int nMajor, int longLimit, int far, int hot, int32_t* cold) {
  GSTRIDE(r, nMajor) {
    const int p0 = beg[r], len = beg[r + 1] - beg[r];
    int c = 0;
    if (len >= 2 && len <= longLimit) {
      const int mid = idx[p0 + len / 2];
      for (int p = p0; p < p0 + len; ++p) {
        const int j = idx[p];
        const int d = j > mid ? j - mid : mid - j;
        if (d >= far && count[j] <= hot) ++c;
      }
    }
    cold[r] = c;
  }
}

void gpuSlabPartition(const DeviceCsrData& M, int32_t longLimit, int32_t majorCost, hipStream_t s, DeviceSlabLayout& L) {
  // the partition by work is sequential and cheap: on the host, from the major starts (4 bytes per major over PCIe),
  // by the same function the host-side build uses
  std::vector<int32_t> hb((size_t)M.nMajor + 1), hc((size_t)std::max(M.nMajor, 1), 0);
  DeviceArray<int32_t> count, cold;
  count.alloc((size_t)std::max(M.nMinor, 1));
  cold.alloc(hc.size());
  count.zero(s);
  if (M.nnz > 0) hipLaunchKernelGGL(k_minor_count, dim3(gridFor(M.nnz)), dim3(kT), 0, s, M.idx.get(), M.nnz, count.get());
  if (M.nMajor > 0)
    hipLaunchKernelGGL(k_major_cold, dim3(gridFor(M.nMajor)), dim3(kT), 0, s, M.beg.get(), M.idx.get(), count.get(), M.nMajor, longLimit,
                       kSlabFar, kSlabHotCount, cold.get());
  M.beg.download(hb.data(), hb.size(), s);
  if (M.nMajor > 0) cold.download(hc.data(), (size_t)M.nMajor, s);
  PDLP_HIP(hipStreamSynchronize(s));
  SlabPartition P = slabPartition(hb.data(), hc.data(), M.nMajor, M.nMinor, longLimit, majorCost);
  L.rowsPerBlock = P.maxRowsPerBlock;
  L.nBlocks = P.nBlocks;
  L.minorBits = P.minorBits;
  L.hostWaveBeg = std::move(P.waveBeg);
  L.waveBeg.alloc(L.hostWaveBeg.size());
  L.waveBeg.upload(L.hostWaveBeg.data(), L.hostWaveBeg.size(), s);
  PDLP_HIP(hipStreamSynchronize(s));
}

void gpuBuildSlabLayout(const DeviceCsrData& M, int32_t longLimit, int32_t W, int32_t majorCost, hipStream_t s, DeviceSlabLayout& L) {
  const int32_t nMajor = M.nMajor, nMinor = M.nMinor;
  const int64_t nnz = M.nnz;
  if (L.hostWaveBeg.empty()) gpuSlabPartition(M, longLimit, majorCost, s, L);
  const int32_t nWaves = L.nBlocks * kSlabWavesPerBlock;
  DeviceArray<int32_t> waveOf;
  waveOf.alloc((size_t)std::max(nMajor, 1));
  if (nMajor > 0) hipLaunchKernelGGL(k_wave_of, dim3(gridFor(nMajor)), dim3(kT), 0, s, L.waveBeg.get(), nWaves, nMajor, waveOf.get());
  const int32_t S = std::max(1, (int32_t)(((int64_t)nMinor + ((int64_t)1 << W) - 1) >> W));
  const int64_t nSeg = (int64_t)nWaves * S;
  if (nSeg >= (int64_t)0x7fffffff) throw std::runtime_error("slab layout: too many segments");
  const uint32_t keyMax = (uint32_t)nSeg;  // sorts after every real segment

  // long majors: mask, map, compact CSR
  const int nWords = (nMajor + 31) / 32 + 1;
  L.longMask.alloc((size_t)nWords);
  DeviceArray<int32_t> longFlag, longRank;
  longFlag.alloc((size_t)std::max(nMajor, 1));
  longRank.alloc((size_t)std::max(nMajor, 1));
  hipLaunchKernelGGL(k_long_mask, dim3(gridFor(std::max(nWords, nMajor))), dim3(kT), 0, s, M.beg.get(), nMajor,
                     longLimit, nWords, L.longMask.get(), longFlag.get());
  exclusiveSum(longFlag.get(), longRank.get(), nMajor, s);
  L.nLong = nMajor > 0 ? fetchOne(longRank.get() + (nMajor - 1), s) + fetchOne(longFlag.get() + (nMajor - 1), s) : 0;
  L.longMap.alloc((size_t)std::max(L.nLong, 1));
  L.longCsr.nMajor = L.nLong;
  L.longCsr.nMinor = nMinor;
  L.hostLongBeg.assign(1, 0);
  if (L.nLong > 0) {
    DeviceArray<int32_t> longLen;
    longLen.alloc(L.nLong);
    hipLaunchKernelGGL(k_long_rows, dim3(gridFor(nMajor)), dim3(kT), 0, s, M.beg.get(), longFlag.get(), longRank.get(),
                       nMajor, L.longMap.get(), longLen.get());
    std::vector<int32_t> hl(L.nLong);
    longLen.download(hl.data(), L.nLong, s);
    PDLP_HIP(hipStreamSynchronize(s));
    L.hostLongBeg.resize((size_t)L.nLong + 1);
    for (int32_t c = 0; c < L.nLong; ++c) L.hostLongBeg[c + 1] = L.hostLongBeg[c] + hl[c];
    const int64_t nnzLong = L.hostLongBeg[L.nLong];
    L.longCsr.nnz = nnzLong;
    L.longCsr.beg.alloc((size_t)L.nLong + 1);
    L.longCsr.beg.upload(L.hostLongBeg.data(), (size_t)L.nLong + 1, s);
    L.longCsr.idx.alloc((size_t)nnzLong + 1);
    L.longCsr.val.alloc((size_t)nnzLong + 1);
    L.longCsr.idx.zero(s);
    L.longCsr.val.zero(s);
    hipLaunchKernelGGL(k_long_copy, dim3(L.nLong), dim3(kT), 0, s, M.beg.get(), M.idx.get(), M.val.get(),
                       L.longMap.get(), L.longCsr.beg.get(), L.longCsr.idx.get(), L.longCsr.val.get());
    PDLP_HIP(hipStreamSynchronize(s));
  } else {
    L.longCsr.nnz = 0;
    L.longCsr.beg.alloc(1);
    L.longCsr.beg.zero(s);
    L.longCsr.idx.alloc(1);  // (the pad element alone: zero, as the host build uploads it)
    L.longCsr.val.alloc(1);
    L.longCsr.idx.zero(s);
    L.longCsr.val.zero(s);
  }

  // short entries sorted by (wave, slab); the stable sort keeps (major, minor) order inside
  DeviceArray<uint32_t> keys, sortedKeys;
  DeviceArray<int32_t> perm;
  keys.alloc((size_t)std::max<int64_t>(nnz, 1));
  if (nnz > 0)
    hipLaunchKernelGGL(k_slab_keys, dim3(gridFor(nnz)), dim3(kT), 0, s, M.beg.get(), M.major.get(), M.idx.get(), nnz,
                       waveOf.get(), S, W, longLimit, keyMax, keys.get());
  sortByKey(keys.get(), nnz, (uint64_t)keyMax, sortedKeys, perm, s);
  L.wavePtr.alloc((size_t)nWaves + 1);
  hipLaunchKernelGGL(k_wave_ptr, dim3(gridFor(nWaves + 1)), dim3(kT), 0, s, sortedKeys.get(), nnz, nWaves, S,
                     L.wavePtr.get());
  L.nnzShort = fetchOne(L.wavePtr.get() + nWaves, s);
  L.ent.alloc((size_t)L.nnzShort + 1);
  L.val.alloc((size_t)L.nnzShort + 1);
  L.ent.zero(s);
  L.val.zero(s);
  if (L.nnzShort > 0)
    hipLaunchKernelGGL(k_slab_entries, dim3(gridFor(L.nnzShort)), dim3(kT), 0, s, perm.get(), M.major.get(),
                       M.idx.get(), M.val.get(), L.nnzShort, waveOf.get(), L.waveBeg.get(), L.minorBits, L.ent.get(), L.val.get());
  PDLP_HIP(hipStreamSynchronize(s));
}

}  // namespace pdlp
