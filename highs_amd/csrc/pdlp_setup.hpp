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

// What a Hessian-updatable solver keeps of a device-side extraction: pdlp_host.hpp HessianMap's arrays in HBM, sized as
// Solver::keepHessian sizes its uploads (an empty array holds one element), and the unscaled diagonal and values of N
// (qdiag0 only where no MatrixKeep holds it).
struct DeviceHessianMap {
  int32_t nSlots = 0, nOff = 0;
  DeviceArray<int32_t> dstBeg, srcSlot, offRow, offCol;
  DeviceArray<double> qdiag0, qoff0;
  bool kept() const { return dstBeg.size() != 0; }
};

// Where a QP's Hessian is extracted.  A pure host function of what the caller knows before any launch; 0 = on the device
// (gpuExtractHessian), anything else = by the host walk (pdlp_host.hpp extractHessian / extractHessianKept), and why.
enum : int32_t {
  kHessOnDevice = 0,
  kHessHostSetup = 1,   // the set-up itself runs on the host
  kHessSharded = 2,     // neither downloadForm nor the shard cut carries N
  kHessHipdlp = 3,      // the HiPDLP form takes no Hessian
  kHessNoSlots = 4,     // q_dim <= 0, no q_start, or q_start[q_dim] <= 0
  kHessStarts = 5,      // q_start[0] != 0 or q_start decreases somewhere: the host walk defines what that means
  kHessSwitchOff = 6,   // PDLP_MI355X_GPU_HESSIAN=0
};
int32_t hessianExtractionReason(bool gpuSetup, bool sharded, bool hipdlp, bool switchOn, int32_t qDim, const int32_t* qStart);

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
  // every slot kept (pdlp_host.hpp extractHessianKept).  Host extraction: its assembly map, the unscaled diagonal and the
  // unscaled values of N stay on the host for the solver to take.  Device extraction (gpuExtractHessian): they stay in HBM
  // — kmap; hmap, hQdiag0 and hQoff0 are then empty
  bool keepHessianPattern = false;
  HessianMap hmap;
  std::vector<double> hQdiag0, hQoff0;
  DeviceHessianMap kmap;
  // The Hessian's extraction (hessianExtractionReason): the caller says what the rule cannot see from the problem — may it
  // run on the device at all (not sharded, the switch PDLP_MI355X_GPU_HESSIAN not 0) — and reads what happened: the
  // rule's reason code (kHessOnDevice: gpuExtractHessian ran), the taken slots and the slots of N, the most HBM the
  // extraction's temporaries held at once (stage "hessian_extraction")
  bool hessianSharded = false, hessianSwitchOn = true;
  int32_t hessianReason = kHessNoSlots;
  int64_t hessianTaken = 0, hessianOffSlots = 0, hessianTempBytes = 0;
  // wall seconds of three parts of gpuPrepare (cuPDLP-C form; stage "setup_seconds"): the Hessian's extraction, the
  // upload that goes with it (host extraction: its diagonal and N; device extraction: the caller's q_start, q_index,
  // q_value), the scaling passes
  double secExtract = 0, secUploadHessian = 0, secPasses = 0;
};

// Options of the HiPDLP form (pdlp_host.hpp formulateHipdlp / scaleHipdlp); nullptr = cuPDLP-C form.
struct HipdlpSetup {
  bool ruiz = true, pc = true, l2 = false;
  int ruizIters = 10;
};
// The caller's arrays in HBM, as the set-up reads them: gpuPrepare's uploads (ownStart / ownIndex then own a_start /
// a_index, which a matrix-updatable solver takes over), or the arrays a device-resident entry was given (pdlp_resident.hpp;
// nothing is owned, what is kept is copied).  hessian: the Hessian's arrays where they are in HBM already, else nullptr.
struct DeviceHessianInputs {
  const int32_t *qStart = nullptr, *qIndex = nullptr;
  const double* qValue = nullptr;
  DeviceArray<int32_t> ownStart, ownIndex;  // gpuExtractHessian's uploads: temporaries of the extraction
  DeviceArray<double> ownValue;
};
struct DeviceInputs {
  const int32_t *aStart = nullptr, *aIndex = nullptr;
  const double *aValue = nullptr, *colCost = nullptr, *colLower = nullptr, *colUpper = nullptr, *rowLower = nullptr, *rowUpper = nullptr;
  DeviceArray<int32_t> ownStart, ownIndex;
  DeviceHessianInputs* hessian = nullptr;
};
// Formulate + scale + both orientations on the device.  Throws std::runtime_error.  gpuPrepare = validate + upload +
// gpuPrepareFromDevice, which reads of P only the sizes, the scalars and HOST copies of a_start, col_cost, row_lower,
// row_upper and q_start; every other array is taken from `in`.
void gpuPrepare(const pdlp_problem_t& P, bool doScale, hipStream_t s, DeviceProblem& out,
                const HipdlpSetup* hipdlp = nullptr);
void gpuPrepareFromDevice(const pdlp_problem_t& P, DeviceInputs& in, bool doScale, hipStream_t s, DeviceProblem& out,
                          const HipdlpSetup* hipdlp = nullptr);
// The Hessian's extraction on the device, for gpuPrepare (pdlp_setup.hip; the rule above decides).  On entry the host's
// own checks have passed (q_dim <= num_col, no null array) and q_start runs from 0 to q_start[q_dim] > 0 without
// decreasing.  Writes D.qdiag and D.N (unscaled, with the sense) exactly as an upload of extractHessian's /
// extractHessianKept's result would, D.kmap when D.keepHessianPattern, the counts and the two times; throws the host
// walk's sentences.  Everything runs on s; synchronises.
void gpuExtractHessian(const pdlp_problem_t& P, int32_t n, hipStream_t s, DeviceProblem& D);
// gpuExtractHessian = upload + this; reads of P only q_dim and a HOST copy of q_start, the slots from `in`
void gpuExtractHessianFromDevice(const pdlp_problem_t& P, DeviceHessianInputs& in, int32_t n, hipStream_t s, DeviceProblem& D);

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
