// k_optsim3.hip -- Optimizer::OptimizeSim3 (src/Optimizer.cc:1116-1323) as ONE launch: both rounds, their Levenberg
// iterations, the lambda trials of every iteration, both classifications and the "fewer than 10 left" exit run inside
// k_optimize_sim3, one problem (loop candidate) per 64-lane workgroup, i.e. per wave.  The arithmetic is optsim3_math.h on
// g2o_math.h: binary64, and the build has -ffp-contract=off, so every product and sum rounds where it is written.
//
// Layout.  No LDS and no barrier.  Lane l owns pairs l, l + 64, ...: it alone reads and writes their `bad` byte and their two
// stored chi2.  A pass evaluates the pairs that are not erased at one transform -- a FULL pass at the estimate (errors,
// chi2, Huber weights, Jacobians; 28 + 7 + 1 sums) or a TRIAL pass at a trial (robust chi2 only) -- and stores each pair's
// two chi2: the classifications read what the LAST pass left, accepted trial or not, as g2o's chi2() does.  Summation order,
// a function of n only: each lane adds its pairs in ascending order, e12 then e21 of a pair; the 64 lanes combine by
// __shfl_down with offsets 32, 16, 8, 4, 2, 1.  Every lane then takes the totals FROM LANE 0 and runs the Levenberg step on
// them redundantly: all lanes hold the same bits, so loop counts, accept / reject and the stop rules are wave-uniform by
// construction and no branch depends on a per-lane copy that might differ.
#include <hip/hip_runtime.h>

#include "optsim3_kernels.h"

namespace orbfe {
namespace {

// the sums of the wave in the fixed order of the header comment, the same bits in every lane on return
template <int K>
__device__ __forceinline__ void wave_sum(double (&acc)[K]) {
#pragma unroll
  for (int k = 0; k < K; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
    acc[k] = __shfl(v, 0);
  }
}

__device__ __forceinline__ int wave_count(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
  return __shfl(v, 0);
}

__device__ __forceinline__ void load_pair(const OptSim3Args& a, int i, OptSim3Pair* p) {
  const float4 A = a.pairA[i], B = a.pairB[i], C = a.pairC[i];
  const float fa[4] = {A.x, A.y, A.z, A.w}, fb[4] = {B.x, B.y, B.z, B.w}, fc[4] = {C.x, C.y, C.z, C.w};
  optsim3_unpack(fa, fb, fc, p);
}

__global__ __launch_bounds__(kOptSim3Threads) void k_optimize_sim3(OptSim3Args a) {
  const int lane = threadIdx.x;
  const OptSim3Problem& pr = a.prob[blockIdx.x];
  OptSim3Result* res = a.res + blockIdx.x;
  const int n = pr.n, first = pr.off, last = pr.off + pr.n;
  const OptSim3Cam K1 = {(double)pr.cam1[0], (double)pr.cam1[1], (double)pr.cam1[2], (double)pr.cam1[3]};
  const OptSim3Cam K2 = {(double)pr.cam2[0], (double)pr.cam2[1], (double)pr.cam2[2], (double)pr.cam2[3]};
  const double delta = (double)pr.delta;
  const float th2 = pr.th2;
  const bool fixScale = pr.fixScale != 0;

  G2oLM<7> lm;
  OptSim3Vertex vx;
  vx.fixScale = fixScale;
  optsim3_from_record(pr.sim3, &vx.est);

  int rounds = 0, nBad = 0, nIn = 0, maxIt = 5;  // optimizer.optimize(5) (:1263)
  bool early = true;                             // the call returns 0 and g2oS12 stays what came in
  if (lane == 0) {
#pragma unroll
    for (int r = 0; r < 2; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
  }

  if (n > 0) {
    for (int i = first + lane; i < last; i += kOptSim3Threads) a.bad[i] = 0;
#pragma unroll 1
    for (int rnd = 0; rnd < 2; rnd++) {
      g2o_lm_begin(&lm, maxIt);
      int cmd = kG2oLMFull;
#pragma unroll 1
      while (cmd != kG2oLMDone) {
        OptSim3Eval E;
        if (cmd == kG2oLMFull) {
          // computeActiveErrors + activeRobustChi2 + buildSystem (optimization_algorithm_levenberg.cpp:75-87)
          optsim3_eval_at(vx.est, &E);
          double acc[kOptSim3Sums];
#pragma unroll
          for (int k = 0; k < kOptSim3Sums; k++) acc[k] = 0.0;
#pragma unroll 1
          for (int i = first + lane; i < last; i += kOptSim3Threads) {
            if (a.bad[i] != 0) continue;
            OptSim3Pair p;
            load_pair(a, i, &p);
            double c12, c21;
            optsim3_pair_full(E, K1, K2, p, delta, fixScale, acc, &c12, &c21);
            a.chi12[i] = c12;
            a.chi21[i] = c21;
          }
          wave_sum<kOptSim3Sums>(acc);
#pragma unroll
          for (int k = 0; k < kOptSim3Sums; k++) lm.S[k] = acc[k];
          cmd = g2o_lm_after_full(&lm);
          optsim3_lm_propose(&lm, &vx);
        } else {
          // computeActiveErrors + activeRobustChi2 at the trial (:123-124)
          optsim3_eval_at(vx.trial, &E);
          double sum[1] = {0.0};
#pragma unroll 1
          for (int i = first + lane; i < last; i += kOptSim3Threads) {
            if (a.bad[i] != 0) continue;
            OptSim3Pair p;
            load_pair(a, i, &p);
            double c12, c21;
            optsim3_pair_trial(E, K1, K2, p, delta, &sum[0], &c12, &c21);
            a.chi12[i] = c12;
            a.chi21[i] = c21;
          }
          wave_sum<1>(sum);
          cmd = g2o_lm_after_trial(&lm, sum[0], &vx.est, vx.trial, [&] { optsim3_lm_propose(&lm, &vx); });
          // the counters are the same in every lane: kept in scalar registers, they leave the vector file to the sums
          cmd = __builtin_amdgcn_readfirstlane(cmd);
          lm.it = __builtin_amdgcn_readfirstlane(lm.it); lm.q = __builtin_amdgcn_readfirstlane(lm.q);
          lm.trials = __builtin_amdgcn_readfirstlane(lm.trials); lm.nBadLM = __builtin_amdgcn_readfirstlane(lm.nBadLM);
        }
      }
      // classification (src/Optimizer.cc:1267-1284, :1302-1316): chi2() reads the error of the last evaluated trial
      int erased = 0, kept = 0;
      for (int i = first + lane; i < last; i += kOptSim3Threads) {
        if (a.bad[i] != 0) continue;
        if (optsim3_is_bad(a.chi12[i], a.chi21[i], th2)) {
          a.bad[i] = (uint8_t)(rnd + 1);
          erased++;
        } else {
          kept++;
        }
      }
      erased = wave_count(erased);
      kept = wave_count(kept);
      if (lane == 0) { res->iterations[rnd] = lm.it; res->trials[rnd] = lm.trials; res->lambda[rnd] = lm.lam; res->chi2[rnd] = lm.cur; }
      rounds = rnd + 1;
      if (rnd == 0) {
        nBad = erased;
        maxIt = nBad > 0 ? 10 : 5;                // nMoreIterations (:1287-1291)
        if (n - nBad < kOptSim3MinPairs) break;   // return 0 (:1293-1294)
      } else {
        nIn = kept;
        early = false;
      }
    }
  }

  if (lane == 0) {
    if (early) optsim3_from_record(pr.sim3, &vx.est);  // (converted again: kept, it would hold 16 registers throughout)
#pragma unroll
    for (int k = 0; k < 4; k++) res->sim3[k] = vx.est.q[k];
#pragma unroll
    for (int k = 0; k < 3; k++) res->sim3[4 + k] = vx.est.t[k];
    res->sim3[7] = vx.est.s;
    res->nIn = nIn; res->nBad = nBad; res->rounds = rounds; res->pad = 0;
  }
}

}  // namespace

void launch_optimize_sim3(hipStream_t s, const OptSim3Args& a, int nProblems) {
  if (nProblems <= 0) return;
  hipLaunchKernelGGL(k_optimize_sim3, dim3(nProblems), dim3(kOptSim3Threads), 0, s, a);
}

}  // namespace orbfe
