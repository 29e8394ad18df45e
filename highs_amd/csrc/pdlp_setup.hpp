// pdlp_setup.hpp — GPU-side problem preparation: the work that
// the reference does on the host before the first PDHG iteration —
// formulateLP_highs (CupdlpWrapper.cpp:280-448), Ruiz + Pock-Chambolle scaling
// (cupdlp_scaling.c), both matrix orientations (cupdlp_cs.c:189) — plus this
// library's slab layouts, done on the device.  At 1M x 1M / 8M nnz the host
// path costs ~1.2 s on the GPU box (the reference: ~1.5 s), i.e. thousands of
// GPU iterations; here it is a few radix sorts and streaming passes.
//
// The results are BIT-IDENTICAL to the host path (pdlp_host.cpp), which is
// itself bit-identical to the oracle and the reference: every reduction whose
// order matters (Pock-Chambolle row/column sums) is done by one thread per
// major in the reference's traversal order; max-reductions are order-free;
// sqrt and division are IEEE-correct on gfx950.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pdlp_device.hpp"
#include "pdlp_host.hpp"
#include "pdlp_kernels.hpp"

namespace pdlp {

// Compressed matrix in HBM; `major[p]` = major index of entry p (kept for the
// scaling passes and the slab-layout sort).
struct DeviceCsrData {
  DeviceArray<int32_t> beg, idx, major;
  DeviceArray<double> val;
  int32_t nMajor = 0, nMinor = 0;
  int64_t nnz = 0;
};

// What a matrix-updatable solver keeps of the set-up (PDLP_UPDATABLE_MATRIX, pdlp_update.hpp): everything here depends on
// the sparsity pattern and the row kinds only, except the two value scratches and the unscaled data.
struct MatrixKeep {
  int64_t nnz0 = 0;  // the caller's nonzeros (nnz - slack entries)
  DeviceArray<int32_t> aStart, aIndex;           // the caller's column-wise pattern
  DeviceArray<int32_t> cscBeg, cscIdx, cscCol;   // reference-order columns (equality-type entries first): row, column of every entry
  DeviceArray<int32_t> aBeg, aMajor, aIdx;       // rows with ascending column
  DeviceArray<int32_t> permA;                    // row-major slot -> reference-order slot
  DeviceArray<int32_t> permAt;                   // column-major (ascending row) slot -> row-major slot; released once the
                                                 // layouts' source indices are composed with it
  DeviceArray<double> cscVal, aVal;              // value scratch of both orders (scaled values after set-up / an update)
  DeviceArray<double> cost0, lower0, upper0, rhs0, qdiag0;  // the UNSCALED formulated data (qdiag0: QP only)
  size_t bytes() const {
    return sizeof(int32_t) * (aStart.size() + aIndex.size() + cscBeg.size() + cscIdx.size() + cscCol.size() + aBeg.size() +
                              aMajor.size() + aIdx.size() + permA.size() + permAt.size()) +
           sizeof(double) * (cscVal.size() + aVal.size() + cost0.size() + lower0.size() + upper0.size() + rhs0.size() + qdiag0.size());
  }
};

struct DeviceProblem {
  int32_t n = 0, m = 0, n0 = 0, nEqs = 0;
  int64_t nnz = 0;
  bool scaled = false;
  double offset = 0.0, sense = 1.0;
  DeviceCsrData A;   // rows, ascending column
  DeviceCsrData At;  // columns, ascending row
  DeviceArray<double> cost, rhs, lower, upper, colScale, rowScale;
  DeviceArray<double> qdiag;      // QP only (cuPDLP-C form): diagonal of Q with the sense, scaled with the columns
  // QP whose Hessian has an off-diagonal part (cuPDLP-C form): N = both triangles by rows with ascending column, in the
  // order the host extraction defines (pdlp_host.hpp extractHessian / extractHessianKept), values scaled with the
  // columns; nnz = 0: none.  idx / val end in the one pad element the layout builds expect.
  DeviceCsrData N;
  DeviceArray<double> rowUpper;   // HiPDLP form only (rhs then holds the row lower bounds)
  DeviceArray<uint8_t> rowIsEq;   // HiPDLP form only, per permuted row
  // host copies of what the host side of the solver needs
  std::vector<int32_t> rowKind, rowNewIdx;
  std::vector<double> hColScale, hRowScale;
  double normCost = 0, normRhs = 0, matNormInf = 0;
  double sumCost2 = 0, sumRhs2 = 0;  // left-to-right sums of the SCALED c, b (PDHG_Init_Step_Sizes)
  // Updatable solvers (set keepPasses before gpuPrepare; cuPDLP-C form only): the scale factors of every pass, pass-major
  // as StandardForm::csPass / rsPass, copied device-to-device out of the pass's temporaries
  bool keepPasses = false;
  int32_t nPass = 0;
  DeviceArray<double> csPass, rsPass;
  // Matrix-updatable solvers (set keepMatrix before gpuPrepare; cuPDLP-C form only): the pattern-only arrays the set-up
  // otherwise frees, both sort permutations and the unscaled data
  bool keepMatrix = false;
  MatrixKeep keep;
  // PDLP_UPDATABLE_HESSIAN (set keepHessianPattern before gpuPrepare; cuPDLP-C form only): the Hessian is extracted with
  // every slot kept (pdlp_host.hpp extractHessianKept); its assembly map, the unscaled diagonal and the unscaled values
  // of N stay on the host for the solver to take
  bool keepHessianPattern = false;
  HessianMap hmap;
  std::vector<double> hQdiag0, hQoff0;
  // wall seconds of three parts of gpuPrepare (cuPDLP-C form; stage "setup_seconds"): the Hessian's extraction on the
  // host, the upload of its diagonal and of N, the scaling passes
  double secExtract = 0, secUploadHessian = 0, secPasses = 0;
};

// Options of the HiPDLP form (pdlp_host.hpp formulateHipdlp / scaleHipdlp); nullptr = cuPDLP-C form.
struct HipdlpSetup {
  bool ruiz = true, pc = true, l2 = false;
  int ruizIters = 10;
};
// Formulate + scale + both orientations on the device.  Throws std::runtime_error.
void gpuPrepare(const pdlp_problem_t& P, bool doScale, hipStream_t s, DeviceProblem& out,
                const HipdlpSetup* hipdlp = nullptr);

// ---- the value-dependent layer of gpuPrepare, shared with pdlp_mi355x_update_matrix (pdlp_update.cpp) ----------------
// The formulated values of the caller's a_value in reference order: <= rows negated, -1.0 for the nSlack slack entries
// behind them.  Pattern arrays as gpuPrepare built them; writes cscVal only.
void gpuFormulateValues(const int32_t* aStart, const int32_t* aIndex, const double* aValue, const int32_t* rowKind,
                        const int32_t* rowNewIdx, int32_t n0, int32_t m, int64_t nnz0, int64_t nSlack, double* cscVal,
                        hipStream_t s);
// The scaling passes of the cuPDLP-C form (Ruiz x 10 in the infinity norm, then Pock-Chambolle alpha = 1): column
// factors from the reference-order columns, row factors from the rows, both copies and the data take each pass.
struct ScaleOperands {
  int32_t n = 0, m = 0;
  int64_t nnz = 0;
  const int32_t *cscBeg = nullptr, *cscIdx = nullptr, *cscCol = nullptr;
  double* cscVal = nullptr;
  const int32_t *aBeg = nullptr, *aMajor = nullptr, *aIdx = nullptr;
  double* aVal = nullptr;
  double *cost = nullptr, *lower = nullptr, *upper = nullptr, *rhs = nullptr, *colScale = nullptr, *rowScale = nullptr;
  double* qdiag = nullptr;                        // QP only, else nullptr
  // the off-diagonal part N of a QP's Hessian: row, column and value of every slot; every pass gives each slot the two
  // divisions (v / cs[row]) / cs[col] of applyScaling.  qoffVal == nullptr: no such part, nothing is launched for it
  const int32_t *qoffRow = nullptr, *qoffCol = nullptr;
  double* qoffVal = nullptr;
  int64_t qoffCount = 0;
  double *csPass = nullptr, *rsPass = nullptr;    // updatable solvers: [11 n], [11 m], pass-major; else nullptr
};
int32_t gpuScalePasses(const ScaleOperands& o, hipStream_t s);  // returns the number of passes (11); synchronises
double gpuAbsMax(const double* val, int64_t count, hipStream_t s);  // max |val[p]| (matNormInf); synchronises
void gpuFill(double* a, double v, int64_t count, hipStream_t s);

// Slab layout (pdlp_host.hpp SlabLayout) built on the device from a device CSR.
struct DeviceSlabLayout {
  int32_t rowsPerBlock = 0, nBlocks = 0, minorBits = 0, nLong = 0;  // rowsPerBlock: most majors in one block
  int64_t nnzShort = 0;
  std::vector<int32_t> hostWaveBeg;  // the partition (pdlp_host.hpp slabPartition), computed on the host from the major starts
  DeviceArray<int32_t> wavePtr, waveBeg;
  DeviceArray<uint32_t> ent, longMask;
  DeviceArray<double> val;
  DeviceCsrData longCsr;            // compacted long majors (major[] unused)
  DeviceArray<int32_t> longMap;     // compact index -> major
  std::vector<int32_t> hostLongBeg; // for the stream plan of the side kernel
};
// gpuSlabPartition: the partition alone (nBlocks, minorBits, rowsPerBlock, hostWaveBeg, waveBeg); gpuBuildSlabLayout
// computes it itself when `out` does not hold one yet.
void gpuSlabPartition(const DeviceCsrData& M, int32_t longLimit, int32_t majorCost, hipStream_t s, DeviceSlabLayout& out);
void gpuBuildSlabLayout(const DeviceCsrData& M, int32_t longLimit, int32_t slabWidthLog2, int32_t majorCost, hipStream_t s,
                        DeviceSlabLayout& out);

}  // namespace pdlp
