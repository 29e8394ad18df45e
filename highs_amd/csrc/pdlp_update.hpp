// pdlp_update.hpp — re-solving a held problem after its costs, bounds or right-hand side changed (pdlp_mi355x_update).
//
// In the cuPDLP-C scheme the scale factors come from the matrix alone (pdlp_host.cpp scale(): Ruiz x 10 + Pock-Chambolle
// look only at the matrix values); cost, bounds and rhs are merely carried along, one pass at a time (applyScaling:
// cost /= cs, lower *= cs, upper *= cs, rhs /= rs).  Row order, slack columns and the sign flip of <= rows depend only on
// each row's KIND.  So with the kinds unchanged and the factors of every pass kept, new data are brought to exactly the
// bits a fresh create() on the modified problem has by REPLAYING the passes in order — dividing once by the accumulated
// colScale does not give the same bits (tests/test_update_host.py shows a case).  The replay runs on the device
// (pdlp_update.hip); hostReplayUpdate restates it for the CPU tests.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pdlp_host.hpp"

namespace pdlp {

// Which parts of the standard form an update touches.
enum : int32_t { kUpdCost = 1, kUpdColLower = 2, kUpdColUpper = 4, kUpdRows = 8 };
inline int32_t updateMask(const pdlp_update_t& u) {
  return (u.col_cost ? kUpdCost : 0) | (u.col_lower ? kUpdColLower : 0) | (u.col_upper ? kUpdColUpper : 0) |
         (u.row_lower && u.row_upper ? kUpdRows : 0);
}

// What can be checked without the problem: row bounds come in pairs, a start is whole or absent.  Throws.
void checkUpdateShape(const pdlp_update_t& u);
// Throws for the smallest row whose kind under the new bounds differs from rowKind (names the row and both kinds); the
// second form is for a row the device's validation kernel has found already.
void refuseKindChange(const int32_t* rowKind, int32_t m, const double* rowLower, const double* rowUpper);
[[noreturn]] void refuseKindChangeAt(const int32_t* rowKind, int32_t row, const double* rowLower, const double* rowUpper);
// ... from that row's kept kind and its two new bounds alone (the arrays are in HBM: pdlp_batch_resident.hpp)
[[noreturn]] void refuseKindChangeAt(int32_t kindWas, int32_t row, double lower, double upper);

// The refusals that depend on how the solver was created, each sentence in ONE place; `entry` is the C entry that refuses.
constexpr const char* kEntryUpdate = "pdlp_mi355x_update";
constexpr const char* kEntryUpdateMatrix = "pdlp_mi355x_update_matrix";
constexpr const char* kEntryUpdateValues = "pdlp_mi355x_update_values";
[[noreturn]] void refuseHipdlp(const char* entry);
[[noreturn]] void refuseSharded(const char* entry);
[[noreturn]] void refuseNotUpdatable(const char* entry);
[[noreturn]] void refuseNoMatrixBit(const char* entry);  // (update_values: "a_value given, but ..." in front)
[[noreturn]] void refuseNoHessianBit(const char* entry);
[[noreturn]] void refuseOffDiagonalHessian(const char* entry);

// The caller's five data arrays in one staging buffer (Solver::updIn_, sessIn_): cost | col_lower | col_upper | row_lower |
// row_upper, count(n0, m) doubles.
struct DataStage {
  double *cost, *colLower, *colUpper, *rowLower, *rowUpper;
  static size_t count(int32_t n0, int32_t m) { return (size_t)3 * n0 + (size_t)2 * m; }
  static DataStage over(double* base, int32_t n0, int32_t m) {
    DataStage d;
    d.cost = base; d.colLower = d.cost + n0; d.colUpper = d.colLower + n0;
    d.rowLower = d.colUpper + n0; d.rowUpper = d.rowLower + m;
    return d;
  }
};

// Host restatement of the device replay on a form that kept its passes (StandardForm::keepPasses): F.cost / lower / upper
// / rhs, normCost / normRhs and offset become those of formulate + scale on the modified problem.  Validates first; throws
// without touching F.
void hostReplayUpdate(const pdlp_update_t& u, StandardForm& F);

// ---- device (pdlp_update.hip) --------------------------------------------------------------------------------------
// bad[0] = min(bad[0], smallest row whose kind changes); the caller sets bad[0] = m first
void launchUpdateValidate(const double* rowLower, const double* rowUpper, const int32_t* rowKind, int32_t m, int32_t* bad,
                          hipStream_t s);
// Columns j < n of the formulated problem.  Original columns (j < n0) take colCost[j] * sense, colLower[j], colUpper[j]
// (each only where mask says its array was given; beyond +-1e20 is infinite); slack column n0 + k takes the bounds of
// row slackRow[k] when mask has kUpdRows.  Then the nPass passes csPass[p * n + j] are replayed in order.
void launchUpdateCols(int32_t mask, const double* colCost, const double* colLower, const double* colUpper,
                      const double* rowLower, const double* rowUpper, const int32_t* slackRow, double sense, int32_t n0,
                      int32_t n, const double* csPass, int32_t nPass, double* cost, double* lower, double* upper, hipStream_t s);
// Original rows i < m: rhs[rowNewIdx[i]] by kind, then rhs /= rsPass[p * m + rowNewIdx[i]] in order.
void launchUpdateRows(const double* rowLower, const double* rowUpper, const int32_t* rowKind, const int32_t* rowNewIdx,
                      int32_t m, const double* rsPass, int32_t nPass, double* rhs, hipStream_t s);


// ---- pdlp_mi355x_update_matrix (PDLP_UPDATABLE_MATRIX) -----------------------------------------------------------------
// New matrix VALUES on the pattern the solver was created with.  Of create()'s work only a thin layer looks at the values:
// the formulated values (sign of <= rows), the scaling passes, matNormInf, the scaled data (every factor changes) and the
// value arrays of the layouts.  Row order, both transposes, slab partitions and sorts, slab width, XCD map, pacing, task
// plans and the captured graph depend on the pattern alone and are kept; none of width / map / pacing changes a sum, so
// whatever a fresh create() would time to, the bits are the same.  A matrix-updatable solver therefore keeps the pattern
// in both orders, the permutation between them, a SOURCE INDEX per value slot of every layout and the unscaled data
// (pdlp_setup.hpp MatrixKeep), and an update is: formulate values -> the set-up's own pass loop (gpuScalePasses) -> one
// refill kernel per value array.  hostReplayMatrixUpdate restates it for the CPU tests.

// F: formulate(P) [+ scale] with keepPasses set and F.cost0 / lower0 / upper0 / rhs0 / qdiag0 holding the unscaled data
// (keepUnscaled).  Afterwards F is formulate + scale of the problem with a_value and u's data (finalize is the caller's),
// its passes and unscaled copies are the new ones.  Validates first; throws without touching F.
void keepUnscaled(StandardForm& F);
// qValue (or nullptr): new Hessian values as well, for a form that also kept its Hessian (keepUnscaledHessian)
void hostReplayMatrixUpdate(const pdlp_problem_t& P, const double* aValue, const pdlp_update_t* u, bool doScale, StandardForm& F,
                            const double* qValue = nullptr);
// The checks both sides share: a_value present, num_nz that of create, not all zero (create's wording).  Throw.
void checkMatrixUpdateShape(const double* aValue, int64_t numNz, int64_t nnzAtCreate);
[[noreturn]] void throwAllZeroMatrix();

// dst[q] = src[q] >= 0 ? val[src[q]] : 0 for q < count (val has nVal elements; an index outside it counts as a pad)
void launchRefill(const int32_t* src, const double* val, int64_t count, int64_t nVal, double* dst, hipStream_t s);
// val[q] = q + 1: values that name their slot, for building the layouts of a matrix-updatable solver
void launchTagValues(double* val, int64_t count, hipStream_t s);
// a layout's value array built from tagged values -> its source indices; slots >= nReal are pads (-1); compose (or
// nullptr): src = compose[tag - 1].  *nTagged (device) += the slots that held a tag: the caller checks that the value
// arrays of an operand hold every entry exactly as often as the matrix has entries
void launchTagsToSource(const double* tags, int64_t count, int64_t nReal, int64_t nVal, const int32_t* compose, int32_t* src,
                        unsigned long long* nTagged, hipStream_t s);


// ---- pdlp_mi355x_update_values (PDLP_UPDATABLE_HESSIAN) -----------------------------------------------------------------
// New Hessian VALUES on the pattern the solver was created with, alone or together with new matrix values and data.  The
// scale factors come from the matrix alone, so with the matrix unchanged a new Q is brought into scaled form by replaying
// the kept column factors of every pass — q_jj -> (q_jj / cs_p[j]) / cs_p[j], q_ij -> (q_ij / cs_p[i]) / cs_p[j], the
// operations applyScaling does — with no scaling pass, no norm, no layout build and the captured graph kept.  When the
// matrix changes too, the same replay with the NEW factors rescales the off-diagonal part (the diagonal rides along with
// the passes as in create).  A Hessian-updatable solver keeps: the assembly map from the caller's slots to the diagonal
// and the row-ordered both-triangle off-diagonal part (pdlp_host.hpp HessianMap), qoff's row and column per slot, the
// unscaled qdiag0 / qoff0, and a source index per value slot of dQ_'s layouts (by the tagged-values construction of the
// matrix update).  hostReplayHessianUpdate restates the Hessian-only case for the CPU tests; with a matrix update the
// Hessian goes through hostReplayMatrixUpdate's scale().
void keepUnscaledHessian(StandardForm& F);  // F.qdiag0, F.qoff0 from a form made by formulate(P, F, true), before scale()
// q_value present iff counted, count that of create, a solver with a Hessian.  Throws.
void checkHessianUpdateShape(const double* qValue, int64_t numQNz, bool hasHessian, int64_t slotsAtCreate);
[[noreturn]] void throwNegativeDiagonal(int32_t col);
// validates (negative diagonal), then F.qdiag0 / F.qoff0 / F.qdiag / F.qoff.val become those of the new values, scaled
// by the kept passes.  Throws without touching F.
void hostReplayHessianUpdate(const double* qValue, StandardForm& F);
// the same validation and assembly into F.qdiag0 / F.qoff0 only (the matrix update's scale() does the rest)
void hostAssembleHessianUpdate(const double* qValue, StandardForm& F, bool validateOnly);

// ---- a value update validated ahead of time (a batch validates every variant before it changes a lane) ------------------
// What the refusals that look at no VALUE depend on: a held solver fills it from itself (Solver::validateValues), the host
// tests from the problem and the options (batchVariantRefusal, pdlp_batch.hpp).
struct ValueUpdateFacts {
  bool sharded = false;
  int32_t updatable = 0;        // pdlp_params_t.updatable as the solver was created with
  int64_t nnz = 0, qSlots = 0;  // the caller's nonzeros and Hessian slots at create (qSlots: 0 without a Hessian)
  bool hasQoff = false;         // the Hessian has an off-diagonal part
  const int32_t* rowKind = nullptr;
  int32_t m = 0;
};
// Throws what pdlp_mi355x_update_values(aValue, numNz, qValue, numQNz, &u) — or pdlp_mi355x_update_matrix(aValue, numNz,
// &u) where that is the entry (a_value alone on a solver without PDLP_UPDATABLE_HESSIAN) — refuses before it looks at a
// value, in that entry's order and words: sharded, the updatable bits, the counts, the off-diagonal Hessian, u's shape
// and the kind change.
void refuseValueUpdate(const ValueUpdateFacts& f, const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz,
                       const pdlp_update_t& u);

// bad[0] = min(bad[0], smallest column whose assembled diagonal is negative); the caller sets bad[0] = n first
void launchHessianValidate(const int32_t* dstBeg, const int32_t* srcSlot, const double* qValue, double sense, int32_t n,
                           int32_t* bad, hipStream_t s);
// qdiag0[j] / qoff0[k] from the caller's slots times sense, summed in extractHessian's order
void launchHessianAssemble(const int32_t* dstBeg, const int32_t* srcSlot, const double* qValue, double sense, int32_t n,
                           int32_t nOff, double* qdiag0, double* qoff0, hipStream_t s);
// qdiag = qdiag0 and qoff = qoff0 taken through the nPass passes csPass[p * n + .]; a part whose source is nullptr is skipped
void launchHessianReplay(const double* qdiag0, const double* qoff0, const int32_t* offRow, const int32_t* offCol, int32_t n,
                         int32_t nOff, const double* csPass, int32_t nPass, double* qdiag, double* qoff, hipStream_t s);

}  // namespace pdlp
