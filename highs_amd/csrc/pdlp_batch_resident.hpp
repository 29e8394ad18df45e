// pdlp_batch_resident.hpp — a batch whose variants and solutions are arrays already in HBM (pdlp_mi355x_batch_run_device,
// DESIGN.md section 2j): the value checks of ALL variants of a call in one launch.
//
// A host batch validates every variant on the host, because it can read the arrays.  With the arrays in HBM the per-update
// kernels (k_update_validate, gpuAbsMax, k_hessian_validate) would be queued K times, a synchronisation each, before the
// first lane may change; k_variants_validate takes all K variants in one launch and leaves one record per variant.  The
// rules are those kernels' rules, comparison for comparison:
//   * firstBadRow: the SMALLEST row i with rowKindOf(row_lower[i], row_upper[i]) != rowKind[i]           (else m)
//   * anyNonzero:  1 iff a_value[p] != 0.0 for some p — a NaN is not zero                               (else 0)
//   * firstNegDiag: the SMALLEST column j whose diagonal, summed from 0.0 over the assembly map's sources in map order,
//     each times the sense, is < 0.0                                                                    (else n)
// A job whose pointer is NULL is skipped and leaves its field as initialised.
//
// Turning the records into a refusal is a host function of its own (refuseByRecords), so that it runs on canned records.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>

#include "../../include/pdlp_mi355x.h"

namespace pdlp {

struct VariantJob {  // one variant's arrays in HBM; NULL: not given
  const double *rowLower, *rowUpper, *aValue, *qValue;
};
struct VariantRecord {
  int32_t firstBadRow, anyNonzero, firstNegDiag;  // initialised to {m, 0, n}
};
struct VariantsValidateArgs {
  const VariantJob* jobs;  // [K], in HBM
  int32_t K;
  const int32_t* rowKind;                  // [m] the kept kinds (lane 0's); NULL: no row job runs
  const int32_t *dstBeg, *srcSlot;         // the Hessian assembly map (lane 0's); NULL: no Hessian job runs
  double sense;
  int32_t m, n;
  int64_t nnz;
  VariantRecord* rec;  // [K], in HBM, initialised
};
// ONE launch: blockIdx.y walks the variants with stride gridDim.y, blockIdx.x strides over max(m, nnz, n).
void launchVariantsValidate(const VariantsValidateArgs& a, hipStream_t s);

// The first finding in the fixed order — the lowest k; within it row-kind change, all-zero matrix, negative diagonal —
// thrown as "variant k: " + the words of refuseKindChangeAt / throwAllZeroMatrix / throwNegativeDiagonal; returns where
// there is none.  v[k]'s pointers are only asked whether they are NULL (no job: no finding, whatever the record holds).
// rowKind: the host's copy of the kept kinds.  fetchBounds(k, row, &lo, &up): that one row's bounds of variant k.
using FetchRowBounds = std::function<void(int32_t k, int32_t row, double* lo, double* up)>;
void refuseByRecords(int32_t K, const pdlp_variant_t* v, const VariantRecord* rec, const int32_t* rowKind, int32_t m, int32_t n,
                     const FetchRowBounds& fetchBounds);

}  // namespace pdlp
