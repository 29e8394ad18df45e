// pdlp_solver.hpp — device-resident PDHG driver (the MI355X counterpart of
// cuPDLP-C's LP_SolvePDHG / PDHG_Solve, cupdlp_solver.c:899-1498).
#pragma once
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdint>
#include <map>
#include <mutex>
#include <stdexcept>
#include <string>
#include <vector>

#include "pdlp_device.hpp"
#include "pdlp_host.hpp"
#include "pdlp_kernels.hpp"
#include "pdlp_mesh.hpp"
#include "pdlp_round.hpp"
#include "pdlp_setup.hpp"

namespace pdlp {

// Environment switches of a solver, read once at creation (pdlp_solver.cpp DevSwitches::fromEnv); -1 = not set.
struct DevSwitches {
  int graph = -1, forceComm = 0, gpuSetup = -1;
  int slab = -1;          // PDLP_MI355X_SLAB: 0 CSR stream only, 1 slab layout, -1 automatic by the gathered vector's size
  int slabW = 0;          // PDLP_MI355X_SLAB_W: log2 of the slab width (development)
  int xcdMap = -1, slabPace = -1;
  int slabTune = 1;       // PDLP_MI355X_SLAB_TUNE=0 (development): the slab width by rule only, no timing of narrower slabs
  int fusedCoTasks = -1;  // PDLP_MI355X_FUSED_COTASKS: 0 = the fused trial's streaming blocks run the long columns' task passes themselves
  int touchTail = 1;      // PDLP_MI355X_TOUCH_TAIL=0 (development): no touching of the tail columns' operands in front of the fused trial's barrier
  int constCached = -1;   // PDLP_MI355X_CONST_CACHED=0|1 (development): c, l, u of the primal step non-temporal / ordinary loads (default: by size)
  int fused = -1, persistent = -1, xcdLocal = -1, hierBarrier = -1, deviceCheck = -1, checkSmall = -1;
  int persistentQp = -1;  // PDLP_MI355X_PERSISTENT_QP=0: small QPs with off-diagonal Hessian entries keep their launches per trial (LPs, diagonal QPs: not read)
  int gpuHessian = -1;    // PDLP_MI355X_GPU_HESSIAN=0: a device-side set-up extracts a QP's Hessian by the host walk (LPs: not read)
  int persistentHipdlp = -1;  // PDLP_MI355X_PERSISTENT_HIPDLP=0: the HiPDLP path keeps its two launches per Halpern step on small LPs too
  int primalInA = -1;     // PDLP_MI355X_PRIMAL_IN_A: the persistent loop without its P phase (pdlp_small.hip PINA); -1 = where measured faster
  int barrierTimeoutMs = 1000;  // PDLP_MI355X_BARRIER_TIMEOUT_MS: how long a grid barrier / roll call waits for missing workgroups
  int fault = 0;          // PDLP_MI355X_FAULT (tests): 1 = the first persistent launch expects one workgroup too many,
                          // 2 = the 12th fused trial's barrier expects one block too many (both then time out and fall back)
  std::string exchange;
  static DevSwitches fromEnv();
};

// One operand matrix in HBM: CSR stream plan or slab layout for the majors that are summed left to right,
// segment tasks for the long ones (pdlp_host.hpp LongPlan).
struct DeviceMatrix {
  DeviceArray<int32_t> beg, idx, blockBeg, wavePtr, waveBeg;
  DeviceArray<uint32_t> ent, longMask;
  DeviceArray<double> val, slabVal;
  // long majors
  DeviceArray<LongTask> lTasks;
  DeviceArray<double> lSegSum, lContrib;
  DeviceArray<uint32_t> lTicket;
  int32_t nLong = 0, nTasks = 0, longSlots = 0, longGroup = 1, taskGroup = 4;
  // slab layout: size the task workgroups so that every CU gets one (uploadPlans).  Off for the operand whose tasks the
  // fused trial runs inside its streaming blocks (already spread evenly; full groups of 16 keep long columns in LDS)
  bool balanceTaskBlocks = true;
  int32_t majorCost = kSlabMajorCostRows;  // slab partition: work of a major besides its entries (the owner sets kSlabMajorCostCols on its transposed operand)
  int32_t fusedCoTasks = 0;  // MatView::coTaskBlocks (the fused trial's task workgroups), decided by the solver at set-up
  int32_t touchTail = 1;     // MatView::touchTail
  int32_t nMajor = 0, nBlocks = 0;  // nBlocks = CSR stream blocks
  int32_t chunk = kChunk;           // work-plan block size of the CSR stream (spmvChunkFor)
  int64_t nnz = 0;
  bool useSlab = false;
  int32_t noPace = 0;  // slab kernel without the per-group block barrier (SlabMat::noPace), see tuneXcdMap
  int32_t slabWidthLog2 = 0;  // log2 of the slab width the layout was built with (either build; see buildSlabTuned)
  double estRunLen = 1.0;     // estimated run length of equal majors at the widest slabs (device build)
  bool mapTuned = false;      // XCD map / pacing already chosen by timing (with the slab width)
  int32_t xcdMap = 1;  // block -> XCD assignment of the SpMV kernels (pdlp_kernels.hip xcdContiguousBlock), see tuneXcdMap
  SlabMat slab{};
  // Host copies of what a build decides and then forgets (slab layout; a few KB): the minors, the XCD that owns every tile
  // of the gathered vector, the per-block span and entry count of the short majors, the long majors.  Read by the test hook
  // pdlp_mi355x_device_matrix alone.
  int32_t nMinor = 0, tileLog2 = 0;
  std::vector<int8_t> hostTileOwner;
  std::vector<int32_t> hostSpanLo, hostSpanHi, hostSpanCnt, hostLongMap;
  // sw.slab: 0 = CSR stream only, 1 = slab layout, -1 = auto by nMinor
  void upload(const Compressed& c, int32_t nMajor_, int32_t nMinor_, const DevSwitches& sw, hipStream_t s);
  // same, from a matrix that is already in HBM (GPU-side setup); takes M's arrays
  void buildFromDevice(DeviceCsrData& M, const DevSwitches& sw, hipStream_t s);
  MatView view() const;
  int32_t nPartials() const { return (useSlab ? slab.nBlocks : 0) + nBlocks + longSlots; }

 private:
  // hostLongIdx / tileOwner / tileLog2 (slab layout): the minors of the long majors on the host and the XCD that owns each
  // tile of the gathered vector — the segment tasks are dealt to workgroups of the XCD their entries live in (planLong)
  void uploadPlans(const std::vector<int32_t>& hostBeg, int32_t nCsrMajor, const int32_t* longVecIndex, hipStream_t s,
                   const int32_t* hostLongIdx = nullptr, const std::vector<int8_t>* tileOwner = nullptr, int32_t tileLog2 = 0);
  // per-block column span / entry count of the short majors -> do the blocks touch few stretches of the gathered vector densely?
  static bool touchesFewTiles(const std::vector<int32_t>& lo, const std::vector<int32_t>& hi, const std::vector<int32_t>& cnt);
};

// Picks M.xcdMap by timing the plain SpMV out = M * in with both block -> XCD assignments (a few launches; the
// result vector is scratch).  PDLP_MI355X_XCD_MAP=0|1 forces one.
// Returns the time of one plain SpMV with the choice made (ms; 0 for operands too small to time).
float tuneXcdMap(DeviceMatrix& M, const DevSwitches& sw, const double* in, double* out, hipStream_t s);
// M -> `out` like DeviceMatrix::buildFromDevice, plus (slab layout, >= 2^20 nonzeros) the slab width chosen by timing
// the plain SpMV at the rule's width, 2^13 and 2^11 (pdlp_solver.cpp buildSlabTuned holds the measurements behind it).
void buildSlabTuned(DeviceMatrix& out, DeviceCsrData& M, const DevSwitches& sw, hipStream_t s);

class Comm;  // RCCL wrapper (pdlp_comm.cpp)
struct DataStage;          // pdlp_update.hpp
struct ValueUpdateFacts;   // pdlp_update.hpp
struct ResidentProblem;    // pdlp_resident.hpp
struct LaneUnit;           // pdlp_batch.hpp
enum LaneVerdict : int;    // pdlp_batch.hpp

// Host copy of cuPDLP's CUPDLPresobj numbers for one iterate.
struct Residuals {
  double pObj = 0, dObj = 0, gap = 0, relGap = 0, pFeas = 0, dFeas = 0;
  double pInfObj = 0, pInfRes = 1, dInfObj = 0, dInfRes = 1;
};

// What the C ABI drives: one implementation per reference path (cuPDLP-C: Solver below;
// HiPDLP: HalpernSolver, pdlp_halpern.hpp).
class SolverBase {
 public:
  virtual ~SolverBase() = default;
  virtual void run(pdlp_result_t* R) = 0;
  virtual void iterate(int32_t nIters, pdlp_iter_stats_t* st) = 0;
  virtual void reset() = 0;
  virtual void dims(int32_t* n, int32_t* m, int64_t* nnz, int32_t* nEqs) const = 0;
  virtual void getVector(const std::string& name, double* host, int64_t len) = 0;
  virtual void setVector(const std::string& name, const double* host, int64_t len) = 0;
  virtual void stage(const std::string& name, double* out, int32_t cap) = 0;
  virtual double timeKernel(const std::string& name, int32_t reps) = 0;
  // test hook pdlp_mi355x_device_matrix: operand 0 = A by rows, 1 = A' by columns, and the stream its arrays are read on
  virtual const DeviceMatrix* deviceMatrix(int32_t which, hipStream_t* s) const = 0;
  // pdlp_mi355x_update; validates before it changes anything.  Only the cuPDLP-C path takes updates.
  virtual void update(const pdlp_update_t& u);
  // pdlp_mi355x_update_matrix; likewise
  virtual void updateMatrix(const double* aValue, int64_t numNz, const pdlp_update_t* u);
  // pdlp_mi355x_update_values; likewise
  virtual void updateValues(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u);
  // New tolerances, limits and log sink for the runs that follow (pdlp_params_t primal_tol, dual_tol, gap_tol, time_limit,
  // iter_limit, log_level, log_callback, log_ctx); every other field of opt is ignored.  Only the cuPDLP-C path takes them.
  virtual void setRuntimeOptions(const pdlp_params_t& opt);
  // pdlp_mi355x_run_device / pdlp_mi355x_update_device (pdlp_resident.hpp): the four vectors of R, every array of u and
  // a_value / q_value are in HBM on the solver's device.  Only the cuPDLP-C path takes them.
  virtual void runDevice(pdlp_result_t* R);
  virtual void updateDevice(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u,
                            hipStream_t callerStream);
};

class Solver : public SolverBase {
 public:
  Solver(const pdlp_problem_t& P, const pdlp_params_t& opt, int32_t rank, int32_t world, const void* id128);
  // pdlp_mi355x_create_device: the problem's arrays are in HBM on opt.device (pdlp_resident.cpp fills RP's host shadow)
  Solver(ResidentProblem& RP, const pdlp_params_t& opt);
  ~Solver() override;

  void run(pdlp_result_t* R) override;                          // LP_SolvePDHG
  void iterate(int32_t nIters, pdlp_iter_stats_t* st) override;  // fixed-work loop for timing
  void reset() override;                                        // PDHG_Init_Step_Sizes + PDHG_Init_Variables

  void dims(int32_t* n, int32_t* m, int64_t* nnz, int32_t* nEqs) const override;
  void getVector(const std::string& name, double* host, int64_t len) override;
  void setVector(const std::string& name, const double* host, int64_t len) override;
  void stage(const std::string& name, double* out, int32_t cap) override;
  double timeKernel(const std::string& name, int32_t reps) override;
  const DeviceMatrix* deviceMatrix(int32_t which, hipStream_t* s) const override { *s = stream_; return which ? &dAt_ : &dA_; }
  void update(const pdlp_update_t& u) override;  // pdlp_update.cpp
  void updateMatrix(const double* aValue, int64_t numNz, const pdlp_update_t* u) override;  // pdlp_update.cpp
  void updateValues(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz,
                    const pdlp_update_t* u) override;  // pdlp_update.cpp
  void setRuntimeOptions(const pdlp_params_t& opt) override;  // pdlp_session.cpp
  void runDevice(pdlp_result_t* R) override;  // pdlp_resident.cpp
  void updateDevice(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u,
                    hipStream_t callerStream) override;  // pdlp_resident.cpp
  // updateDevice for a caller that has ordered this solver's stream behind the stream the arrays were filled on already
  // (a batch: ONE event for all its lanes, pdlp_batch_resident.hpp): orderBehind false records and waits for nothing
  void updateDeviceBehind(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t* u,
                          hipStream_t callerStream, bool orderBehind);

  // ---- what a session drives (pdlp_session.hpp; all in pdlp_session.cpp) ----
  // The caller's a_value, costs, bounds and (QPs) Hessian arrays into HBM copies of their own, for later comparisons.
  // Needs a solver created with PDLP_UPDATABLE_MATRIX (and PDLP_UPDATABLE_HESSIAN for a problem with Hessian slots).
  void sessionAdopt(const pdlp_problem_t& P);
  // P's arrays into the staging buffers of the updates (and the pattern's), then the comparison pass against the kept
  // copies: *changed = the array bits of PDLP_CHANGED_*, *kindRow = the smallest row whose kind changes or -1 (*kindWas its
  // kept kind), *uploadSeconds = what the uploads alone took.  P has the shape of the held problem (the caller has checked).  Nothing of the solver is written.
  void sessionStage(const pdlp_problem_t& P, int32_t* changed, int32_t* kindRow, int32_t* kindWas, double* uploadSeconds);
  // While set, update / updateMatrix / updateValues take the caller's arrays from the staging buffers as sessionStage left
  // them instead of uploading them again (the host pointers still serve the host-side norms).
  void sessionSetStaged(bool on) { staged_ = on; }
  // After an update from staged arrays: staging and kept copies change places (the kept copy now is P).
  void sessionCommit();
  size_t sessionHeldBytes() const;  // HBM kept for reuse beyond a plain solver's

  // ---- what a batch and a pool drive (pdlp_batch.hpp, pdlp_pool.hpp; all in pdlp_batch_lanes.cpp) ----
  // run() cut into the steps of ONE lane of a batch, whose launches are shared with other solvers of the same problem.
  // The steps are the pieces doSolveDevice is made of (beginDeviceLoop, beginRound, afterRound, endDeviceLoop): laneBegin =
  // run() up to its first round; laneQueue = the units [trial batch][check] of the next round, handed out as launch
  // records and accounted for as if launched (units[0] may be the entry's check alone); laneDownload / laneAfterRound =
  // syncState + the round's verdict; laneFinish = what run() does behind its loop.  Between laneBegin and laneFinish
  // nothing else may be asked of the solver.
  // laneSequentialReason: empty, or why this solver's launches cannot be shared (it then runs alone)
  std::string laneSequentialReason() const;
  bool hasOffDiagonalHessian() const { return hasQoff_; }
  int32_t laneWorkBlocks() const { return smallGrid_; }
  // the refusals of update(u) that do not depend on the device, with update's words; nothing is changed
  void validateUpdate(const pdlp_update_t& u) const;
  // likewise every refusal of updateValues(aValue, numNz, qValue, numQNz, &u) — of updateMatrix where a_value comes alone to
  // a solver without PDLP_UPDATABLE_HESSIAN —, the all-zero matrix and the negative diagonal included; nothing of the
  // solver's problem is changed (the Hessian's values go through the update's own staging buffer and validation kernel)
  void validateValues(const double* aValue, int64_t numNz, const double* qValue, int64_t numQNz, const pdlp_update_t& u) const;
  ValueUpdateFacts valueUpdateFacts() const;  // what those refusals depend on, from this solver (pdlp_update.hpp)
  void laneBegin();
  bool laneIdle() const { return loop_.noLoop; }  // the iteration limit is reached before the first round: laneFinish may follow at once
  void laneQueue(int32_t ahead, std::vector<LaneUnit>& units);
  void laneDownload(hipStream_t shared);  // the state record -> host mirror, behind the round's launches
  LaneVerdict laneAfterRound();           // (the shared stream has been synchronised)
  int32_t laneCommError() const { return loop_.commError; }
  int32_t laneXcc();                      // the XCC id this solver's workers published at their last placement check, or -1
  void laneFinish(pdlp_result_t* R, bool resultOnDevice = false);  // resultOnDevice: R's vectors are in HBM (run_device's post-solve)
  // What the validation launch of a device batch reads of this solver (pdlp_batch_resident.hpp): the kept kinds in HBM and
  // on the host, the Hessian assembly map (NULL: none kept), the sense and the sizes
  struct VariantCheckFacts {
    const int32_t *rowKindDev = nullptr, *rowKindHost = nullptr, *dstBeg = nullptr, *srcSlot = nullptr;
    double sense = 1.0;
    int32_t m = 0, n = 0;
    int64_t nnz = 0;
  };
  VariantCheckFacts laneVariantCheckFacts() const;
  bool laneKeepsMatrix() const { return matrixUpdatable_; }  // what updateDevice asks before it takes an a_value
  hipStream_t laneStream() const { return stream_; }
  // the device gate for a round of shared launches (BarrierRound of doSolveDevice) on a stream the caller names: a batch's
  // lane 0's, or one that is no solver's own (a pool's: its solvers come and go, pdlp_pool.hpp)
  static std::unique_lock<std::mutex> sharedBeginRound(int device, hipStream_t s);
  static void sharedEndRound(int device, hipStream_t s, std::unique_lock<std::mutex>& gate);

 private:
  // setup
  void construct(const pdlp_problem_t& P, const void* id128, ResidentProblem* resident = nullptr);
  void release() noexcept;
  void uploadProblem();
  void uploadProblemFromDevice(DeviceProblem& D);
  void uploadShardFromDevice(DeviceProblem& D);  // sharded, two-all-gathers layout: the rank's shard cut on the device
  static void downloadForm(DeviceProblem& D, StandardForm& F, hipStream_t s);
  void allocIterates();
  void initStepSizes();
  void initVariables();
  void applyHotStart();
  void setHotStart(const double* colValue, const double* rowValue, const double* rowDual);  // -> startX_, startY_ (formulated, scaled)
  void keepForUpdates(DeviceProblem* D);  // updatable solvers: the passes and the row bookkeeping into HBM
  // matrix-updatable solvers (pdlp_update.hpp): the host set-up's pattern into mk_; the operands' values replaced by tags
  // in front of the layout builds; the layouts' source indices out of the tagged builds, and the first refill
  void keepMatrixFromHost(const pdlp_problem_t& P);
  void finishMatrixKeep();
  void refillOperands();
  // Hessian-updatable solvers (pdlp_update.hpp): the assembly map and the unscaled Hessian into hk_; dQ_'s source indices
  // out of its tagged build and the first refill; the parts of an update
  void keepHessian(const std::vector<double>& qdiag0, const std::vector<double>& qoff0);
  void keepHessian(DeviceHessianMap& K);  // device-side extraction: the map and the unscaled Hessian are in HBM already
  void finishHessianKeep(const std::vector<double>& qoffScaled);  // host set-up: the scaled values of N from the form
  void finishHessianKeep(const DeviceArray<double>& qoffScaled);  // device-side set-up: device to device
  void finishHessianKeep(const double* qoffScaled, hipMemcpyKind from);
  void refillHessian();
  void stageHessian(const double* qValue);
  void applyHessian(bool assemble, bool replayDiag);
  void updateImpl(const pdlp_update_t& u, const double* qValue);
  void updateMatrixImpl(const double* aValue, int64_t numNz, const pdlp_update_t* u, const double* qValue);
  // what the two share (pdlp_update.cpp): refusals, HEAD (ensureDataStaging, stageRowsAndValidate, ..., stageColumns), each
  // one's own middle, TAIL (refreshScaledSums, refreshBoundsFlipsUniform, finishUpdate)
  void ensureDataStaging();  // updIn_, updBad_ on first use
  void stagePut(double* dev, const double* host, int64_t count);  // an upload, unless staged_
  void stageRowsAndValidate(const pdlp_update_t& ud, int32_t mask, const DataStage& D);  // throws on a kind change
  void stageColumns(const pdlp_update_t& ud, int32_t mask, const DataStage& D);
  void replayData(int32_t mask, const DataStage& D, const double* csPass, const double* rsPass, int32_t nPass, double* cost,
                  double* lower, double* upper, double* rhs);
  void refreshScaledSums(bool cost, bool rhs);  // sumCost2_ / sumRhs2_ from a download of cost_ / rhs_; one synchronisation
  bool refreshBoundsFlipsUniform();             // refreshBlockBounds(); true: IterVecs::lowerUniform flipped
  void finishUpdate(const pdlp_update_t& ud, bool recapture, double* resetSeconds, double* captureSeconds,
                    std::chrono::steady_clock::time_point t0);
  // stage "update_state" [0], [4], [6]: HBM kept for data / matrix / Hessian updates (sessionHeldBytes adds the session's own)
  size_t dataKeptBytes() const;
  size_t matrixKeptBytes() const;
  size_t hessianKeptBytes() const;
  bool refreshBlockBounds();              // fused slab trial: colBlockUni_ / colBlockBounds_ from lower_ / upper_; returns allLower
  // hot loop
  void enqueueTrial();
  void enqueueBatch(int32_t todo);  // trials up to the next halt: one persistent launch / the captured graph / single trials
  void captureGraph();
  void runUntilHalt();
  void syncState();    // device -> host_
  void pushState(bool wait = true);    // host_ -> device
  // check iteration
  void computeAverage();
  void computeResiduals();
  bool checkTermination(const Residuals& r) const;
  bool checkInfeasibility();
  int restartIterate();  // 0: no restart, 1: to the current iterate, 2: to the average
  int32_t checkInterval() const { return opt_.check_interval > 0 ? opt_.check_interval : kReleaseInterval; }
  int32_t nextCheckIter(int32_t it) const;
  void checkStepSearch(int32_t iterBefore, int32_t trialsBefore);  // throws once 50 stops in a row have accepted no trial
  void doSolve(bool terminate, int32_t iterBudget);        // check iterations driven by the host (sharded paths, profile mode)
  void doSolveDevice(bool terminate, int32_t iterBudget);  // check iterations on the device, several periods queued ahead
  // ... in the pieces a lane of a batch is driven by as well (pdlp_batch_lanes.cpp); their state between the calls is loop_
  bool beginDeviceLoop(bool terminate, int64_t iterLim);  // false: the limit is reached, there is no loop (and no endDeviceLoop)
  RoundPlan beginRound(int32_t ahead);                    // the units to queue now (pdlp_round.hpp)
  bool afterRound(bool pushWaits);                        // the host's look at a finished round; true: queue the next one
  void endDeviceLoop();
  // the records of a persistent trial launch and of a one-launch check, accounted for as launched: every caller's way to them
  SmallTrialsLaunch smallTrialsLaunch(int32_t maxTrials);
  CheckSmallLaunch checkSmallLaunch();
  void finishRun(pdlp_result_t* R, bool resultOnDevice = false);
  void enqueueCheckDevice();
  void uploadCtl(bool terminate, int64_t iterLim);
  void downloadCtl();
  void processRecords(bool terminate, int64_t iterLim, int& logSinceHeader);
  void logCheckLine(int32_t it, const Residuals& cur, const Residuals& avg, double t, int& logSinceHeader) const;
  void postsolve(pdlp_result_t* R);
  void postsolveDevice(pdlp_result_t* R);  // pdlp_resident.cpp: the same bits, the four vectors written in HBM
  void postsolveScalars(pdlp_result_t* R, bool cv, bool cd, bool rv, bool rd);  // what both write to the host struct
  // linear algebra on device (sharding-aware)
  void deviceAx(const double* x, double* axLocal);
  void deviceATy(const double* yLocal, double* aty);
  double reduceScalar(const double* partials, int32_t nBlocks, bool overRanks);
  void sumOverRanks(double* devBuf, int32_t count);  // RCCL all-reduce or mesh rank-ordered sum
  void gatherToHost(const double* devLocal, int32_t lo, int32_t hi, bool byRows, std::vector<double>& full);
  std::pair<double*, int64_t> lookup(const std::string& name);
  void log(int level, const char* fmt, ...) const;
  double elapsed() const;
  bool timeIsUp();  // elapsed() > time_limit, agreed across ranks when sharded (identical control flow)

  pdlp_params_t opt_;
  DevSwitches sw_;
  StandardForm F_;
  bool hasStart_ = false;
  std::vector<double> startX_, startY_;
  // sharding
  int32_t rank_ = 0, world_ = 1, r0_ = 0, r1_ = 0, mLoc_ = 0;
  Comm* comm_ = nullptr;
  bool gpuSetup_ = true;   // formulate/scale/transpose/slab layout on the device (pdlp_setup.hip)
  // device-side set-up: wall seconds of the Hessian's extraction, the upload that goes with it, the scaling passes and N's
  // layout build (stage "setup_seconds"; zeros after a host set-up)
  double setupParts_[4] = {};
  // stage "hessian_extraction": the rule's reason code (pdlp_setup.hpp hessianExtractionReason; 0 = on the device), the
  // taken slots, the slots of N, the most HBM the device extraction's temporaries held at once
  int32_t hessReason_ = kHessNoSlots;
  int64_t hessTaken_ = 0, hessOffSlots_ = 0, hessTempBytes_ = 0;
  double sumCost2_ = 0, sumRhs2_ = 0;  // left-to-right sums of the scaled c, b
  bool sharded_ = false;  // row-block sharded kernel sequence (world > 1, or forced for testing)
  bool shardOnDevice_ = false;  // sharded + device-side set-up: the rank's shard is cut on the device (uploadShardFromDevice)
  // exchange of the sharded path: direct xGMI mesh (pdlp_mesh.hpp; columns are then sliced as
  // well, [c0_, c1_)) or, as the fallback, RCCL all-reduce with replicated column work
  Mesh* mesh_ = nullptr;
  bool meshMode_ = false;
  // Mesh layout: row block for A x, column block A[:, c0:c1) for A'y, two all-gathers per trial (x+ slices, y+ row
  // blocks), no n-length partial.  Every rank then keeps y, yAvg (and the power method's work vector) at FULL length m;
  // yOff_ = r0_ is where its rows sit.  (The round-1 layout — all-gather of x+, reduce-scatter of the A'y partials — has
  // been removed.)
  int32_t yOff_ = 0, yLen_ = 0;
  double* yl(int k) const { return y_[k].get() + yOff_; }
  double* yAvgl() const { return yAvg_.get() + yOff_; }
  double* tmpMl() const { return tmpM_.get() + yOff_; }
  int32_t c0_ = 0, c1_ = 0, nLoc_ = 0;
  IterVecs vecsCol_{};  // vecs_ restricted to the own column slice
  IterVecs vecsAty_{};  // mesh layout: vecsCol_ with the FULL-length y (what the column-block A'y kernel gathers from)
  // device
  hipStream_t stream_ = nullptr;
  DeviceMatrix dA_, dAt_;
  // QP whose Hessian has off-diagonal entries: N = the off-diagonal part (symmetric, scaled with the
  // columns), N x by parity like A'y, N xAvg at checks, the partials of dx . N dx
  DeviceMatrix dQ_;
  bool hasQoff_ = false;
  DeviceArray<double> nx_[2], nxAvg_, partQ_;
  DeviceArray<double> x_[2], y_[2], ax_[2], aty_[2];
  DeviceArray<double> xAvg_, yAvg_, axAvg_, atyAvg_, xSum_, ySum_, xLast_, yLast_;
  DeviceArray<double> cost_, rhs_, lower_, upper_, colScale_, rowScale_, qdiag_;  // qdiag_: QP only
  DeviceArray<double> slackPos_, slackNeg_, slackPosAvg_, slackNegAvg_;
  DeviceArray<double> partDY_, partDX_, partInter_, statPart_, statOut_, commBuf_, tmpM_, gatherBuf_;
  // Two slots: the single-GPU loop alternates between them from trial to trial (k_decide_primal reads
  // one, writes the other); stPar_ = the slot that holds the state after everything enqueued so far.
  DeviceArray<DevState> dState_;
  int32_t stPar_ = 0, graphPar_ = 0;
  // Fused trial (2 launches, pdlp_kernels.hpp launchSpmvAtyFusedPrimal): the A'y kernel also takes the decision and
  // does the next primal step.  needPrimal_: the host has pushed a state since the last trial, so the next trial
  // starts with a stand-alone primal step.
  bool fused_ = false, needPrimal_ = true;
  // Small LPs: a batch of trials is ONE persistent launch (pdlp_small.hip); smallGrid_ = its workgroups
  bool persistent_ = false, xcdLocal_ = false, hierBar_ = false, primalInA_ = false;
  // QP with off-diagonal Hessian entries inside the persistent loop: N as its third operand (pdlp_small.hip QOFF)
  mutable SmallQp smallQp_{};
  const SmallQp* smallQp() const {  // (nullptr: an LP or a diagonal QP)
    if (!hasQoff_) return nullptr;
    smallQp_.N = dQ_.view();
    smallQp_.partQ = partQ_.get();
    return &smallQp_;
  }
  const char* qpNotPersistent_ = nullptr;  // why such a QP keeps its launches per trial (laneSequentialReason)
  int smallMode() const { return xcdLocal_ ? 1 : hierBar_ ? 2 : 0; }
  int32_t smallGrid_ = 0;
  DeviceArray<unsigned long long> gridBar_;
  DeviceArray<int32_t> colBlockUni_;     // IterVecs::colBlockUni / colBlockBounds (fused slab launch)
  DeviceArray<double> colBlockBounds_;
  int64_t uniLowerCols_ = 0, uniUpperCols_ = 0;  // columns covered by a block-wide lower / upper bound (stage "uniform_bound_columns")
  // Updatable solvers (pdlp_params_t.updatable, pdlp_update.hpp): the scale factors of every pass (pass-major), the kind
  // and permuted index of every original row, the row behind every slack column; staging for the caller's arrays
  // (allocated by the first update).  updSeconds_: the parts of the last update (stage "update_seconds").
  bool updatable_ = false;
  int32_t nPass_ = 0;
  DeviceArray<double> csPass_, rsPass_, updIn_;
  DeviceArray<int32_t> rowKindDev_, rowNewIdxDev_, slackRowDev_, updBad_;
  // Matrix-updatable solvers (PDLP_UPDATABLE_MATRIX): mk_ (pdlp_setup.hpp MatrixKeep) and, per value array of the two
  // operands' layouts (stream / long-major val, slab val), the slot of mk_.aVal every value slot is filled from (-1: pad).
  // updMat_: staging of the caller's a_value (allocated by the first matrix update).  updMatSeconds_: the parts of the
  // last one (stage "update_matrix_seconds").
  bool matrixUpdatable_ = false;
  int64_t nnzIn_ = 0;  // the caller's nonzeros at create
  MatrixKeep mk_;
  DeviceArray<int32_t> srcAVal_, srcASlab_, srcAtVal_, srcAtSlab_;
  DeviceArray<double> updMat_;
  enum { kMatStage, kMatFormulate, kMatPasses, kMatRefills, kMatSums, kMatBounds, kMatCapture, kMatReset, kMatSlots };
  double updMatSeconds_[kMatSlots] = {};  // upload + validation, formulate, scaling passes, refills, norms + sums, block bounds, graph capture, reset
  // Hessian-updatable solvers (PDLP_UPDATABLE_HESSIAN): the assembly map from the caller's q_value slots (HessianMap), row
  // and column of every qoff slot, the unscaled Hessian (the diagonal lives in mk_.qdiag0 when the solver is matrix-
  // updatable as well), the scaled off-diagonal values dQ_ is refilled from, and per value array of dQ_'s layouts the qoff
  // slot every value slot is filled from.  updQ_: staging of the caller's q_value (allocated by the first Hessian update).
  bool hessianUpdatable_ = false;
  struct HessianKeep {
    int32_t nSlots = 0, nOff = 0;
    DeviceArray<int32_t> dstBeg, srcSlot, offRow, offCol;
    DeviceArray<double> qdiag0, qoff0, qoffScaled;
    size_t bytes() const {
      return sizeof(int32_t) * (dstBeg.size() + srcSlot.size() + offRow.size() + offCol.size()) +
             sizeof(double) * (qdiag0.size() + qoff0.size() + qoffScaled.size());
    }
  } hk_;
  double* qdiag0Dev() { return matrixUpdatable_ ? mk_.qdiag0.get() : hk_.qdiag0.get(); }
  DeviceArray<int32_t> srcQVal_, srcQSlab_;
  DeviceArray<double> updQ_;
  enum { kHessStage, kHessAssemble, kHessReplay, kHessRefill, kHessSlots };
  double updHessSeconds_[kHessSlots] = {};  // upload + validation, assembly, replay, refill of dQ_ (stage "update_values_seconds")
  int32_t updRecaptured_ = 0;                // 1 = the last update captured the trial graph again
  // Session-held solvers (pdlp_session.hpp): the caller's arrays of the last call (sessIn_ laid out as updIn_, sessMat_ as
  // updMat_, sessQ_ as updQ_, sessQPat_ = q_start then q_index), staging of the pattern (a_start, a_index, q_start,
  // q_index), the comparison's record and its pinned mirror.  staged_: see sessionSetStaged.
  bool staged_ = false;
  DeviceArray<double> sessIn_, sessMat_, sessQ_;
  DeviceArray<int32_t> sessQPat_, updPat_, sessRec_;
  int32_t* hostRec_ = nullptr;
  int32_t sessQDim_ = 0;
  // run_device (pdlp_resident.hpp): the rank among the ranged-or-free rows of every original row and, for a solver that is
  // not updatable (rowKindDev_ / rowNewIdxDev_ are then empty), its kind and permuted index — uploaded by the first
  // run_device (the kinds never change: an update that would change one is refused); stage "update_state" does not count them
  DeviceArray<int32_t> postKind_, postNewIdx_, postRank_;
  enum { kUpdStage, kUpdKernels, kUpdSums, kUpdBounds, kUpdCapture, kUpdReset, kUpdSlots };
  double updSeconds_[kUpdSlots] = {};  // upload + validation, kernels, norms + sums, block bounds, graph capture, reset
  int32_t barrierFallbacks_ = 0, smallLaunches_ = 0;
  unsigned long long smallSeq_ = 0;  // persistent launches since gridBar_ was zeroed (their roll call counts cumulatively)
  // (barrier rounds of the contexts of one device: ordered on the DEVICE by an event chain, see pdlp_solver.cpp)
  struct DeviceGate { std::mutex mu; hipEvent_t ev[2] = {nullptr, nullptr}; int cur = 0; bool recorded = false; };
  static DeviceGate& deviceGate(int device);
  std::unique_lock<std::mutex> beginBarrierRound();          // locked (and the stream ordered behind the last round) iff this solver launches grid barriers
  void endBarrierRound(std::unique_lock<std::mutex>& gate);  // marks the end of this round on the stream, releases the gate
  struct BarrierRound {  // a round in scope: ended (event recorded, gate released) on every way out, also by an exception
    Solver& self;
    std::unique_lock<std::mutex> gate;
    ~BarrierRound();
  };
  int32_t stalledRounds_ = 0, stalledSince_ = 0;  // consecutive device stops without an accepted trial
  struct DeviceLoop {  // a device-driven loop between its pieces: beginDeviceLoop .. endDeviceLoop
    RoundLoop sched{};
    int64_t seq0 = 0;                                 // the round under way: its first check, the counters in front of it
    int32_t iterBefore = 0, trialsBefore = 0;
    int32_t commError = 0;                            // (a lane: why it left its shared launches)
    int logSinceHeader = 50;
    bool noLoop = false, timeUp = false;
  } loop_;
  // Device-driven check iterations (pdlp_kernels.hpp CheckCtl; PDLP_MI355X_DEVICE_CHECK=0 gives the host-driven loop back)
  bool devCheck_ = true;
  DeviceArray<CheckCtl> dCtl_;
  CheckCtl* hostCtl_ = nullptr;      // pinned staging copy
  CheckRecord* hostRing_ = nullptr;  // pinned: one record per queued check, written by the device
  static constexpr int32_t kRingSlots = 64;
  int64_t checkSeq_ = 0, checkSeen_ = 0;  // checks enqueued / records looked at
  DeviceArray<double> partRestartY_;
  // Small LPs: the check as ONE launch (pdlp_check.hip k_check_small); its barrier words and launch counter
  bool checkSmall_ = false;
  DeviceArray<unsigned long long> checkBar_;
  unsigned long long checkSmallSeq_ = 0;
  DevState* dst() const { return dState_.get() + stPar_; }
  DeviceArray<double> powRed_, powGrow_;  // host-tabulated powers of the trial counter (see DevState)
  void refreshPowTable();
  DevState* hostState_ = nullptr;  // pinned mirror
  double* hostStats_ = nullptr;    // pinned
  int32_t statStride_ = 0;
  IterVecs vecs_{};
  // scalar solver state (host side of CUPDLPresobj / CUPDLPiterates)
  Residuals cur_, avg_;
  double pFeasLR_ = 0, dFeasLR_ = 0, gapLR_ = 0, pFeasLC_ = 0, dFeasLC_ = 0, gapLC_ = 0;
  int32_t iLastRestartIter_ = 0, nRestarts_ = 0, nChecks_ = 0;
  int32_t lastRestartKind_ = 0, lastCheckIter_ = -1;  // of the last check, host- or device-driven (stage "restart_state")
  int32_t termCode_ = PDLP_TERM_TIMELIMIT_OR_ITERLIMIT, termIterate_ = 0;
  bool adaptive_ = true, restartOn_ = true;
  double feasTol_ = 1e-8;
  std::chrono::steady_clock::time_point solveBeg_;
  double setupSeconds_ = 0, solveSeconds_ = 0;
  // optional hipGraph of a batch of trials
  hipGraphExec_t graphExec_ = nullptr;
  int32_t graphTrials_ = 0;
  bool useGraph_ = true;
  // in-loop kernel timing (stage "profile_on"): HIP events around the two SpMV launches of every trial
  bool profile_ = false;
  std::vector<hipEvent_t> profEvents_;
  int32_t profTrialsQueued_ = 0;
  double profAxMs_ = 0, profAtyMs_ = 0;
  int64_t profLaunches_ = 0;
  void profCollect(int32_t realTrials);
};

// RCCL communicator, loaded lazily with dlopen so that the library itself has
// no link-time dependency on librccl.
class Comm {
 public:
  static void uniqueId(void* id128);
  Comm(int32_t rank, int32_t world, const void* id128);
  ~Comm();
  void allReduceSum(double* buf, size_t count, hipStream_t s);
  int32_t rank() const { return rank_; }
  int32_t world() const { return world_; }

 private:
  void* comm_ = nullptr;
  int32_t rank_, world_;
};

}  // namespace pdlp
