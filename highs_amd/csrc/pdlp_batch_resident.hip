// pdlp_batch_resident.hip — the value checks of all variants of a pdlp_mi355x_batch_run_device call in ONE launch (see
// pdlp_batch_resident.hpp), in the shape of k_session_diff (pdlp_session.hip): several jobs per launch, every array read
// once, unit-stride, with non-temporal loads (the updates that follow stream them again from HBM; nothing here is worth a
// cache line's stay), nothing stored, and a wave reduction in front of the three integer atomics — so a record sees at
// most one atomicMin / atomicOr / atomicMin per wave.  Integer min and or are order-free: the records do not depend on
// how the grid is scheduled.  No floating-point operation besides the comparisons and the diagonal's sum, which runs in
// one thread, in map order, as k_hessian_validate (pdlp_update.hip) runs it; -ffp-contract=off like every other unit.
#include "pdlp_batch_resident.hpp"

#include <algorithm>
#include <climits>
#include <stdexcept>
#include <string>

#include "pdlp_device.hpp"
#include "pdlp_devfn.hpp"
#include "pdlp_host.hpp"
#include "pdlp_update.hpp"

namespace pdlp {

namespace {

constexpr int kT = 256;
constexpr int kMaxBlocks = 2048;   // 256 CUs x 8 resident blocks of 256 threads; the rest is the grid-stride loops'
constexpr int kMaxVariantsY = 16;  // variants side by side; more are walked with stride gridDim.y

__global__ __launch_bounds__(kT) void k_variants_validate(const VariantsValidateArgs A) {
  const int64_t tid = (int64_t)blockIdx.x * kT + threadIdx.x;
  const int64_t stride = (int64_t)gridDim.x * kT;
  for (int32_t k = (int32_t)blockIdx.y; k < A.K; k += (int32_t)gridDim.y) {
    const VariantJob job = A.jobs[k];  // (uniform across the block: scalar loads)
    int32_t bad = INT_MAX, any = 0, neg = INT_MAX;
    if (job.rowLower && job.rowUpper && A.rowKind) {  // the rule of k_update_validate
      for (int64_t i = tid; i < A.m; i += stride)
        if (rowKindOf(ldStream(job.rowLower + i), ldStream(job.rowUpper + i)) != ldStream(A.rowKind + i)) bad = min(bad, (int32_t)i);
    }
    if (job.aValue) {  // gpuAbsMax(...) == 0.0 as the host states it: some value != 0.0 (a NaN is not zero)
      const double* a = job.aValue;
      int64_t p = tid;
      for (; p + 3 * stride < A.nnz; p += 4 * stride) {  // four independent loads in flight per thread and trip
        const double a0 = ldStream(a + p), a1 = ldStream(a + p + stride), a2 = ldStream(a + p + 2 * stride), a3 = ldStream(a + p + 3 * stride);
        any |= (a0 != 0.0) | (a1 != 0.0) | (a2 != 0.0) | (a3 != 0.0);
      }
      for (; p < A.nnz; p += stride) any |= ldStream(a + p) != 0.0;
    }
    if (job.qValue && A.dstBeg && A.srcSlot) {  // the rule of k_hessian_validate
      for (int64_t j = tid; j < A.n; j += stride) {
        const int b = ldStream(A.dstBeg + j), e = ldStream(A.dstBeg + j + 1);
        double d = 0.0;
        for (int q = b; q < e; ++q) d += job.qValue[A.srcSlot[q]] * A.sense;
        if (d < 0.0) neg = min(neg, (int32_t)j);
      }
    }
#pragma unroll
    for (int off = kWave / 2; off > 0; off >>= 1) {
      bad = min(bad, __shfl_xor(bad, off, kWave));
      any |= __shfl_xor(any, off, kWave);
      neg = min(neg, __shfl_xor(neg, off, kWave));
    }
    if ((threadIdx.x & (kWave - 1)) == 0) {
      VariantRecord* r = A.rec + k;
      if (bad != INT_MAX) atomicMin(&r->firstBadRow, bad);
      if (any) atomicOr(&r->anyNonzero, 1);
      if (neg != INT_MAX) atomicMin(&r->firstNegDiag, neg);
    }
  }
}

}  // namespace

void launchVariantsValidate(const VariantsValidateArgs& a, hipStream_t s) {
  if (a.K <= 0) return;
  const int64_t most = std::max<int64_t>({(int64_t)a.m, a.nnz, (int64_t)a.n});
  if (most <= 0) return;
  const int gy = std::min<int>(a.K, kMaxVariantsY);
  const int gx = (int)std::max<int64_t>(1, std::min<int64_t>((most + kT - 1) / kT, kMaxBlocks / gy));
  hipLaunchKernelGGL(k_variants_validate, dim3(gx, gy), dim3(kT), 0, s, a);
  PDLP_HIP(hipGetLastError());
}

void refuseByRecords(int32_t K, const pdlp_variant_t* v, const VariantRecord* rec, const int32_t* rowKind, int32_t m, int32_t n,
                     const FetchRowBounds& fetchBounds) {
  for (int32_t k = 0; k < K; ++k) {
    try {
      const VariantRecord& r = rec[k];
      if (v[k].u.row_lower && v[k].u.row_upper && r.firstBadRow >= 0 && r.firstBadRow < m) {
        double lo = 0.0, up = 0.0;
        fetchBounds(k, r.firstBadRow, &lo, &up);
        refuseKindChangeAt(rowKind[r.firstBadRow], r.firstBadRow, lo, up);
      }
      if (v[k].a_value && r.anyNonzero == 0) throwAllZeroMatrix();
      if (v[k].q_value && r.firstNegDiag >= 0 && r.firstNegDiag < n) throwNegativeDiagonal(r.firstNegDiag);
    } catch (const std::exception& e) {
      throw std::runtime_error("variant " + std::to_string(k) + ": " + e.what());
    }
  }
}

}  // namespace pdlp
