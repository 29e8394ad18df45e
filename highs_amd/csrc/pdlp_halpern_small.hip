// pdlp_halpern_small.hip — the Halpern steps kFirst..kLast of a HiPDLP block on a SMALL LP as ONE persistent launch.
//
// A Halpern step (hipdlp/pdhg.cc:961-1018) is two SpMVs with element-wise epilogues and nothing else: no reduction, no
// accept / reject, no step-size change inside a block.  As plain launches (launchHalpernPrimal, launchHalpernDual) the 39
// steps between a block's first step and its check are 78 kernel nodes whatever the LP's size; on an LP of a few dozen work
// blocks the kernel boundaries are most of that time.  Here a few dozen resident workgroups run them inside one launch:
//     P  A' y_current with the primal projection, reflection and blend     writes rx, xc (major step: xn, slack)
//     D  A reflected_x with the dual ones                                  writes yc     (major step: yn, ry)
// Phase P gathers yc, which phase D wrote; phase D gathers rx, which phase P wrote: a step is P | barrier | D | barrier
// (the barrier behind the launch's last phase is the kernel's end).  The last step is the block's major one.
//   Bits: a workgroup owns the same 512-entry block of A' and of A for the whole launch (OwnBlock: entries, values and the
// bookkeeping of the lane's first major in registers, as in the trial loop of pdlp_small.hip); work blocks, lane assignment
// and the left-to-right major sums are k_spmv's, and the epilogue is THE function the plain launches call (pdlp_devfn.hpp
// halpernPrimal / halpernDual, which differ between the two forms only in the store policy they are given).  The library
// is built without floating-point contraction, so one function in two kernels computes the same bits.
//   Access rule: every vector written inside the launch — xc, yc, rx, and on the major step xn, yn, ry, slack — is read and
// written through ldM / stM, the owner's re-read of its own xc / yc in the next step included: agent-scope accesses on all
// XCDs (MODE 0), or ordinary stores and non-temporal loads on ONE XCD (MODE 1, every eighth workgroup of the launch works;
// the XCC-id placement check runs in every launch, the nt-load self-test once per solver — both as in the trial loop).
// Anchors, cost, bounds, row bounds, the matrix and its plans are constant for the launch: ordinary loads, and those of
// a lane's first major stay in registers.  Every wave drains its stores (s_waitcnt vmcnt(0), then the block barrier)
// before the workgroup's arrival word is written.
//   FROZEN ARGUMENTS.  The launch is replayed from captured graphs (the unit of the device-driven loop, the block of the
// host-driven one): its kernel arguments never change.  So nothing that differs between two launches is an argument,
// and HalpernState::hIter — which restarts from zero at every restart — numbers nothing.  The choice made here: a MEMSET
// NODE in front of every launch zeroes the arrival words, the timeout flag, the roll-call word, the XCC ids and the
// self-test's words (launchHalpernSmall queues it with the launch), the roll call then always waits for `grid` arrivals
// and the barriers of a launch count their epochs 1, 2, ... from the launch's start.  The two words that must outlive a
// launch (self-test passed; a test's request to stall) lie behind the zeroed range and are read from memory at entry.
//   Failure handling.  Entry: the state record goes to LDS; if `halted` or `stalled` is set the launch returns.  Then the
// roll call (pdlp_devfn.hpp rollCall): nothing is written before every working workgroup is known to be resident.  A
// failed roll call (3) or placement check / self-test (2) changes no vector: workgroup 0 sets HalpernState::stalled to the
// code, sets `halted` and clears the gate words run / runFpe0 / doRestart, so that everything queued behind is a no-op —
// as behind a halt, with no change to the plain launches' kernels — until the host has looked; the host then goes on in MODE 0 (2) or with plain launches (3) from the unchanged state.  A barrier can only fail
// behind a passed roll call, on a defect: gridWait's verdict is all-or-none, every workgroup stops stepping at that
// barrier and reports stalled = 1, which ends the solve in an error — never a silently wrong iterate.
//   Out of scope here: the XCD-hierarchical barrier (more than 64 work blocks) and long majors, whose segment tasks are tied
// to the trial loop's partial slots.
#include "pdlp_halpern_small.hpp"

#include <hip/hip_runtime.h>

#include "pdlp_devfn.hpp"

namespace pdlp {

namespace {

struct HalpernSmallArgs {
  SpmvMat A, At;
  HalpernVecs h;
  HalpernState* st;
  unsigned long long* bar;
  int32_t kFirst, kLast;
  unsigned long long limit;  // 100 MHz ticks a roll call or barrier wait may last
};

// arrive (pdlp_devfn.hpp) with the barrier's verdict handed to every thread of the workgroup
template <bool LOCAL>
__device__ __forceinline__ int arriveVerdict(unsigned long long* bar, int lb, int nBlocks, unsigned long long epoch, unsigned long long limit,
                                             int* verdictLds) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // every storing wave drains its stores ...
  __syncthreads();                                    // ... before the block's arrival word is written
  if (threadIdx.x < kWave) {
    const int v = gridBarrier<LOCAL>(bar, lb, nBlocks, epoch, (int)threadIdx.x, limit);
    if (threadIdx.x == 0) *verdictLds = v;
  }
  __syncthreads();
  return *verdictLds;
}

// The launch could not run (or go on): the code for the host — and `halted` with the gate words, so that every kernel of
// every unit still queued is a no-op exactly as behind a halt (the step kernels and k_h_decide look at `halted`, the
// check's kernels and the copies at their gate words); the host un-halts when it has dealt with the code.
__device__ __forceinline__ void reportStall(HalpernState* st, int code) {
  __hip_atomic_store(&st->halted, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->run, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->runFpe0, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->doRestart, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  __hip_atomic_store(&st->stalled, code, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// One phase of a step over the owned block: k_spmv's stream path (same plan, lanes and sums) with the Halpern epilogue.
// fixedPre: the constant operands of the lane's first major (registers); its changing operand (xc / yc) is fetched here.
template <bool PRIMAL, bool LOCAL>
__device__ __forceinline__ void halpernSmallPass(const HalpernVecs& h, const SpmvMat& M, const OwnBlock<kChunkSmall>& B, const Pre& fixedPre,
                                                 double step, double rho, double w, double* prod) {
  constexpr int kPer = kChunkSmall / kSpmvThreads;
  const int tid = threadIdx.x;
  const double* in = PRIMAL ? h.yc : h.rx;     // the gathered vector: written by the other phase
  const double* own = PRIMAL ? h.xc : h.yc;    // this phase's own iterate: written by this phase of the previous step
  const int r1 = B.r1, p0 = B.p0, cnt = B.cnt;
  const int rFirst = B.r0 + tid;
  const int rr = rFirst < r1 ? rFirst : r1 - 1;
  int qb = B.qb, qe = B.qe;
  double xg[kPer];
#pragma unroll
  for (int k = 0; k < kPer; ++k) xg[k] = ldM<LOCAL>(in + B.ci[k]);
  Pre pre = fixedPre;
  pre.a = ldM<LOCAL>(own + rr);
#pragma unroll
  for (int k = 0; k < kPer; ++k) {
    const int q = tid + k * kSpmvThreads;
    if (q < cnt) prod[slot(q)] = B.va[k] * xg[k];
  }
  __syncthreads();
  for (int r = rFirst; r < r1; r += kSpmvThreads) {
    if (r != rFirst) {
      qb = M.beg[r] - p0;
      qe = M.beg[r + 1] - p0;
      pre.a = ldM<LOCAL>(own + r);
      if (PRIMAL) { pre.b = h.cost[r]; pre.c = h.xa[r]; pre.d = h.lower[r]; pre.e = h.upper[r]; }
      else { pre.b = h.ya[r]; pre.c = h.rowLower[r]; pre.d = h.rowUpper[r]; }
    }
    const double s = majorSum(prod, qb, qe);
    if (PRIMAL) halpernPrimal<HalpernIoLoop<LOCAL>>(h, r, s, pre, step, rho, w);
    else halpernDual<HalpernIoLoop<LOCAL>>(h, r, s, pre, step, rho, w);
  }
}

// MODE 0: agent-scope accesses on all XCDs; 1: XCD-local.  Both meet at the flat sweep barrier.
template <int MODE>
__global__ __launch_bounds__(kSpmvThreads) void k_halpern_small(const HalpernSmallArgs a) {
  constexpr bool LOCAL = MODE == 1;
  if (LOCAL && (blockIdx.x & 7) != 0) return;  // XCD-local: every eighth workgroup works
  const int lb = LOCAL ? (int)blockIdx.x >> 3 : (int)blockIdx.x;  // logical workgroup
  const int G = LOCAL ? (int)gridDim.x >> 3 : (int)gridDim.x;
  __shared__ double prod[kChunkSmall + kChunkSmall / 8 + 8];
  __shared__ HalpernState sh;
  __shared__ int verdict;
  __shared__ int entry;          // 0: go on; else the stall code the launch ends with before it has written anything
  __shared__ int needSelfTest;
  const int tid = threadIdx.x;
  static_assert(sizeof(HalpernState) / 4 <= kSpmvThreads && sizeof(HalpernState) % 4 == 0, "state record: one word per thread");
  if (tid < (int)(sizeof(HalpernState) / 4)) reinterpret_cast<uint32_t*>(&sh)[tid] = reinterpret_cast<const uint32_t*>(a.st)[tid];
  padSlots(prod, kChunkSmall + kChunkSmall / 8 + 8, tid, kSpmvThreads);  // (never written again)
  __syncthreads();
  if (sh.halted || sh.stalled) return;
  // The two words that outlive a launch are read BEFORE the roll call: whoever writes one (workgroup 0, behind the self-test's
  // last barrier) does so after every workgroup has passed this point.  Then the roll call: nothing is written before every
  // working workgroup of the launch is known to be resident.
  if (tid < kWave) {
    unsigned long long force = 0ull, tested = 0ull;
    if (tid == 0) {
      force = __hip_atomic_load(a.bar + kHsForceWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tested = __hip_atomic_load(a.bar + kHsTestedWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    const bool here = rollCall(a.bar + G + 1, (unsigned long long)G, a.limit, tid);
    if (tid == 0) {
      // (stage "stall_next_block": the requested code is reported where the real failure would be — 3 here, 2 at the placement check)
      entry = !here || force == 3ull ? 3 : (LOCAL && force == 2ull ? -2 : 0);
      needSelfTest = tested == 0ull ? 1 : 0;
    }
  }
  __syncthreads();
  if (entry == 3) {
    if (lb == 0 && tid == 0) reportStall(a.st, 3);
    return;
  }
  const bool forcePlacement = entry == -2;
  __syncthreads();
  const int nA = a.A.nBlocks, nAt = a.At.nBlocks;
  OwnBlock<kChunkSmall> bA, bAt;
  if (lb < nA) bA.load(a.A, lb, false, nullptr);
  if (lb < nAt) bAt.load(a.At, lb, false, nullptr);
  unsigned long long epoch = 0;
  if (LOCAL) {
    // the placement check: XCC ids of all workers (words behind the arrival words, the timeout flag and the roll-call word)
    unsigned long long* ids = a.bar + G + 8;
    if (tid == 0) __hip_atomic_store(ids + lb, (unsigned long long)xccId() + 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (arriveVerdict<false>(a.bar, lb, G, ++epoch, a.limit, &verdict) != kBarOk) {
      if (tid == 0) reportStall(a.st, 1);
      return;
    }
    if (tid == 0) {
      const unsigned long long mine = __hip_atomic_load(ids + lb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      int ok = forcePlacement ? 0 : 1;
      for (int i = 0; i < G; ++i) ok &= __hip_atomic_load(ids + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == mine;
      entry = ok ? 0 : 2;
    }
    __syncthreads();
    if (entry == 2) {  // nothing has been touched: report, and let the host continue on all XCDs
      if (lb == 0 && tid == 0) reportStall(a.st, 2);
      return;
    }
    if (needSelfTest) {
      // What this mode relies on, checked once per solver on the placement it actually got (as in pdlp_small.hip): a
      // `global_load ... nt` is served by the XCD's L2, never by a line this CU's L1 still holds from an earlier read.  Every
      // workgroup warms its L1 with a plain read of its neighbour's word, the neighbour then stores a new value (plain store,
      // as the loop's stores), and an nt load must return the new value.
      unsigned long long* tw = a.bar + 2 * G + 8;  // G test words, G arrival words, flag, failure word
      unsigned long long* tbar = tw + G;
      unsigned long long* fail = tbar + G + 1;
      const int nb = (lb + 1) % G;
      auto plainLoad = [&](const unsigned long long* p) {
        unsigned long long v;
        asm volatile("global_load_dwordx2 %0, %1, off\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
        return v;
      };
      auto ntLoad = [&](const unsigned long long* p) {
        unsigned long long v;
        asm volatile("global_load_dwordx2 %0, %1, off nt\n\ts_waitcnt vmcnt(0)" : "=v"(v) : "v"(p) : "memory");
        return v;
      };
      int bad = 0;
      if (tid == 0) *reinterpret_cast<volatile unsigned long long*>(tw + lb) = 1ull;
      bad |= arriveVerdict<true>(tbar, lb, G, 1ull, a.limit, &verdict);
      unsigned long long warm = 0;
      if (tid == 0) warm = plainLoad(tw + nb);  // now in this CU's L1
      bad |= arriveVerdict<true>(tbar, lb, G, 2ull, a.limit, &verdict);
      if (tid == 0) *reinterpret_cast<volatile unsigned long long*>(tw + lb) = 2ull;
      bad |= arriveVerdict<true>(tbar, lb, G, 3ull, a.limit, &verdict);
      if (tid == 0 && (warm != 1ull || ntLoad(tw + nb) != 2ull)) __hip_atomic_store(fail, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      bad |= arriveVerdict<true>(tbar, lb, G, 4ull, a.limit, &verdict);
      if (bad != 0) {  // (all-or-none, like every barrier of the launch: a defect, not a placement)
        if (tid == 0) reportStall(a.st, 1);
        return;
      }
      if (tid == 0) entry = __hip_atomic_load(fail, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0ull ? 2 : 0;
      __syncthreads();
      if (entry == 2) {  // an nt load returned a stale line: nothing has been touched, the host continues on all XCDs
        if (lb == 0 && tid == 0) reportStall(a.st, 2);
        return;
      }
      if (lb == 0 && tid == 0) __hip_atomic_store(a.bar + kHsTestedWord, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  // what no step changes: step sizes, the Halpern counter at the block's start, and the constant operands of the lane's first major
  const double tau = sh.tau, sigma = sh.sigma, rho = sh.rho;
  const int hIter = sh.hIter;
  HalpernVecs h = a.h;
  Pre preP{0.0, 0.0, 0.0, 0.0, 0.0}, preD{0.0, 0.0, 0.0, 0.0, 0.0};
  if (bAt.have) {
    const int rF = bAt.r0 + tid, rr = rF < bAt.r1 ? rF : bAt.r1 - 1;
    preP.b = h.cost[rr]; preP.c = h.xa[rr]; preP.d = h.lower[rr]; preP.e = h.upper[rr];
  }
  if (bA.have) {
    const int rF = bA.r0 + tid, rr = rF < bA.r1 ? rF : bA.r1 - 1;
    preD.b = h.ya[rr]; preD.c = h.rowLower[rr]; preD.d = h.rowUpper[rr];
  }
  for (int k = a.kFirst; k <= a.kLast; ++k) {
    h.major = k == a.kLast ? 1 : 0;
    const int kk = hIter + k;  // (Epi<kHalpern*>: hs.hIter + kOff)
    const double w = (double)kk / ((double)kk + 1.0);
    // ---- P: A' y_current, primal projection, reflection, blend ----
    if (bAt.have) halpernSmallPass<true, LOCAL>(h, a.At, bAt, preP, tau, rho, w, prod);
    if (arriveVerdict<LOCAL>(a.bar, lb, G, ++epoch, a.limit, &verdict) != kBarOk) {
      if (tid == 0) reportStall(a.st, 1);
      return;
    }
    // ---- D: A reflected_x, dual projection, reflection, blend ----
    if (bA.have) halpernSmallPass<false, LOCAL>(h, a.A, bA, preD, sigma, rho, w, prod);
    if (k == a.kLast) break;  // (the kernel's end is the barrier behind the last phase)
    if (arriveVerdict<LOCAL>(a.bar, lb, G, ++epoch, a.limit, &verdict) != kBarOk) {
      if (tid == 0) reportStall(a.st, 1);
      return;
    }
  }
}

}  // namespace

int halpernSmallResident(int device) {
  int perCu = 0, cus = 0;
  // (the two modes differ in their accesses only; the agent-scope one is asked about)
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&perCu, reinterpret_cast<const void*>(k_halpern_small<0>), kSpmvThreads, 0) != hipSuccess) return 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess) return 0;
  // (the hardware may admit fewer blocks per CU than the occupancy query says: stay far below, as smallTrialsGrid does)
  return (perCu < 4 ? perCu : 4) * cus;
}

void launchHalpernSmall(const HalpernSmallLaunch& q, int mode, hipStream_t s) {
  (void)hipMemsetAsync(q.bar, 0, halpernSmallZeroedWords(q.grid) * sizeof(unsigned long long), s);
  HalpernSmallArgs a{};
  a.A = q.A.csr; a.At = q.At.csr; a.h = q.h; a.st = q.st; a.bar = q.bar; a.kFirst = q.kFirst; a.kLast = q.kLast;
  a.limit = (unsigned long long)(q.timeoutMs > 0 ? q.timeoutMs : 1000) * 100000ull;
  if (mode == 1) hipLaunchKernelGGL(k_halpern_small<1>, dim3(8 * q.grid), dim3(kSpmvThreads), 0, s, a);
  else hipLaunchKernelGGL(k_halpern_small<0>, dim3(q.grid), dim3(kSpmvThreads), 0, s, a);
}

}  // namespace pdlp
