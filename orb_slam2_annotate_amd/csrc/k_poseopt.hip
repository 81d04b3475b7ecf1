// k_poseopt.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:256-473) as ONE launch: the four rounds, their Levenberg
// iterations and the lambda trials of every iteration run inside k_pose_optimize, one problem per workgroup.  Only the graph
// PoseOptimization builds is covered: one free VertexSE3Expmap, unary EdgeSE3ProjectXYZOnlyPose /
// EdgeStereoSE3ProjectXYZOnlyPose edges, Huber kernel, a dense 6 x 6 system.  All arithmetic is binary64, as in g2o; the
// build has -ffp-contract=off, so every product and sum below rounds where it is written.
//
// The arithmetic is poseopt_math.h on g2o_math.h; this file keeps what is the device's own: the gather of the table form, the
// LDS staging, the reduction, the command / pose broadcast and the round loop.
//
// Layout.  Lane t of the T = 256 lanes owns edges t, t + T, ...: it alone reads and writes their level and stored chi2.  A
// pass over the edges evaluates them at the pose broadcast in LDS -- a FULL pass at the estimate (error, chi2, Huber weight,
// Jacobian; 21 + 6 + 1 sums) or a TRIAL pass at a trial pose (robust chi2 only).  Summation order, a function of (n, T)
// only: each lane adds its edges in ascending order; the 64 lanes of a wave combine by __shfl_down with offsets 32, 16, 8,
// 4, 2, 1; the four wave sums are added in wave order.  Lane 0 then plays OptimizationAlgorithmLevenberg::solve on the
// 6 x 6 system and broadcasts the next pose and the next command.  Mono edges are carried as three-row edges whose third
// row is zero, and edges outside the active set add +0.0: neither changes a sum.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "poseopt_kernels.h"

namespace orbfe {
namespace {

constexpr int kT = kPoseOptThreads;
constexpr int kWaves = kT / 64;
constexpr int kSums = kPoseOptSums;

// the sums of the workgroup in the fixed order of the header comment; out[k] valid for every lane on return
template <int K>
__device__ __forceinline__ void block_sum(double (&acc)[K], double* sPart, double* out, int t) {
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
    if (lane == 0) sPart[wave * K + k] = v;
  }
  __syncthreads();
  if (t < K) {
    double s = sPart[t];
    for (int w = 1; w < kWaves; w++) s = s + sPart[w * K + t];
    out[t] = s;
  }
  __syncthreads();
}

template <bool kLds>
__global__ __launch_bounds__(kPoseOptThreads) void k_pose_optimize(PoseOptArgs a) {
  constexpr int kCap = kLds ? kPoseOptLdsEdges : 1;
  __shared__ float sE[7][kCap];
  __shared__ double sPart[kWaves * kSums];
  __shared__ G2oLM<6> sLM;        // lane 0's Levenberg state; S: H, b, chi2 of the last FULL pass, summed in place
  __shared__ double sChi[1];      // robust chi2 of the last TRIAL pass / outlier count of a classification
  __shared__ PoseOptPose sPose;   // the pose the next pass evaluates
  __shared__ int sCmd;
  __shared__ int sWaveCnt[kWaves];

  const int t = threadIdx.x;
  const PoseOptProblem pr = a.prob[blockIdx.x];
  PoseOptResult* res = a.res + blockIdx.x;
  float4* eA = a.edgeA + pr.off;
  float4* eB = a.edgeB + pr.off;
  uint8_t* level = a.level + pr.off;
  double* chi2s = a.chi2 + pr.off;
  int n = pr.n;

  if (a.gather) {
    // the edges of the table form, in feature order: a feature with a match whose slot is not bad (Optimizer.cc:298-304)
    int base = 0;
    for (int c0 = 0; c0 < pr.n; c0 += kT) {
      const int i = c0 + t;
      int s = -1;
      if (i < pr.n) {
        const int m = a.match[i];
        if (m >= 0) {
          s = a.slot[m];
          if (a.table.flags[s] & ORBFE_MP_BAD) s = -1;
        }
      }
      const unsigned long long mask = __ballot(s >= 0);
      const int lane = t & 63, wave = t >> 6;
      if (lane == 0) sWaveCnt[wave] = __popcll(mask);
      __syncthreads();
      int before = 0, total = 0;
      for (int w = 0; w < kWaves; w++) {
        if (w < wave) before += sWaveCnt[w];
        total += sWaveCnt[w];
      }
      if (s >= 0) {
        const int e = base + before + __popcll(mask & ((1ull << lane) - 1ull));
        const float4 r0 = a.table.rec[2 * (size_t)s];
        eA[e] = make_float4(r0.x, r0.y, r0.z, a.invLevelSigma2[a.featOctave[i]]);
        eB[e] = make_float4(a.featX[i], a.featY[i], a.featUr ? a.featUr[i] : -1.0f, 0.0f);
        a.edgeFeat[e] = i;
      }
      base += total;
      __syncthreads();
    }
    n = base;
    __threadfence_block();
    __syncthreads();
  }

  if (n < 3) {  // nInitialCorrespondences < 3: nothing is touched (Optimizer.cc:385)
    if (t == 0) poseopt_result_untouched(pr, n, res);
    return;
  }

  if (kLds) {
    for (int e = t; e < n; e += kT) {
      const float4 A = eA[e], B = eB[e];
      sE[0][e] = A.x; sE[1][e] = A.y; sE[2][e] = A.z; sE[3][e] = B.x; sE[4][e] = B.y; sE[5][e] = B.z; sE[6][e] = A.w;
    }
  }
  for (int e = t; e < n; e += kT) level[e] = 0;
  __syncthreads();

  auto load = [&](int e, PoseOptEdge* E) {
    if (kLds) {
      E->X[0] = (double)sE[0][e]; E->X[1] = (double)sE[1][e]; E->X[2] = (double)sE[2][e];
      E->u = (double)sE[3][e]; E->v = (double)sE[4][e]; E->ur = (double)sE[5][e]; E->w = (double)sE[6][e];
    } else {
      const float4 A = eA[e], B = eB[e];
      E->X[0] = (double)A.x; E->X[1] = (double)A.y; E->X[2] = (double)A.z;
      E->u = (double)B.x; E->v = (double)B.y; E->ur = (double)B.z; E->w = (double)A.w;
    }
  };

  PoseOptCam C;
  for (int k = 0; k < 5; k++) C.K[k] = (double)pr.K5[k];
  C.deltaMono = (double)a.deltaMono; C.deltaStereo = (double)a.deltaStereo;

  G2oLM<6>& lm = sLM;
  PoseOptPose start, est;  // lane 0's
  int nActive = n, nBad = 0, rounds = 0;
  if (t == 0) poseopt_pose_from_Tcw(pr.Tcw, &start);

  for (int rnd = 0; rnd < 4; rnd++) {
    const bool robust = rnd < 3;  // after round index 2 every edge loses its kernel (Optimizer.cc:429-430, :458-459)
    if (t == 0) {
      est = start;  // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) (:399)
      sPose = est;
      sCmd = nActive > 0 ? kG2oLMFull : kG2oLMDone;  // no active edge: optimize() returns at once (sparse_optimizer.cpp:356)
      g2o_lm_begin(&lm, kPoseOptMaxIt);
    }
    __syncthreads();
    while (true) {
      const int cmd = sCmd;
      if (cmd == kG2oLMDone) break;
      const PoseOptPose P = sPose;
      if (cmd == kG2oLMFull) {
        // computeActiveErrors + activeRobustChi2 + buildSystem (optimization_algorithm_levenberg.cpp:75-87)
        double acc[kSums];
#pragma unroll
        for (int k = 0; k < kSums; k++) acc[k] = 0.0;
        for (int e = t; e < n; e += kT) {
          if (level[e] != 0) continue;
          PoseOptEdge E;
          load(e, &E);
          chi2s[e] = poseopt_edge_full(P, C, E, robust, acc);
        }
        block_sum<kSums>(acc, sPart, lm.S, t);
        if (t == 0) {
          sCmd = g2o_lm_after_full(&lm);
          poseopt_lm_propose(&lm, est, &sPose);
        }
      } else {
        // computeActiveErrors + activeRobustChi2 at the trial (:123-124)
        double acc[1] = {0.0};
        for (int e = t; e < n; e += kT) {
          if (level[e] != 0) continue;
          PoseOptEdge E;
          load(e, &E);
          chi2s[e] = poseopt_edge_trial(P, C, E, robust, &acc[0]);
        }
        block_sum<1>(acc, sPart, sChi, t);
        if (t == 0) {
          const int next = g2o_lm_after_trial(&lm, sChi[0], &est, sPose, [&] { poseopt_lm_propose(&lm, est, &sPose); });
          if (next != kG2oLMTrial) sPose = est;
          sCmd = next;
        }
      }
      __syncthreads();
    }
    // classification (Optimizer.cc:403-463): an outlier edge is recomputed at the estimate, an inlier keeps the error of the
    // last evaluated trial -- rejected or not
    const PoseOptPose P = sPose;
    double cnt[1] = {0.0};
    for (int e = t; e < n; e += kT) {
      PoseOptEdge E;
      load(e, &E);
      double c2;
      if (level[e] != 0) {
        c2 = poseopt_edge_chi2(P, C, E);
        chi2s[e] = c2;
      } else {
        c2 = chi2s[e];
      }
      const bool bad = poseopt_is_outlier(c2, E);
      level[e] = bad ? 1 : 0;
      cnt[0] = cnt[0] + (bad ? 1.0 : 0.0);
    }
    block_sum<1>(cnt, sPart, sChi, t);
    if (t == 0) {
      nBad = (int)sChi[0];
      nActive = n - nBad;
      res->iterations[rnd] = lm.it; res->trials[rnd] = lm.trials; res->lambda[rnd] = lm.lam; res->chi2[rnd] = lm.cur;
      rounds = rnd + 1;
    }
    __syncthreads();
    if (n < 10) break;  // optimizer.edges().size() < 10 (:462)
  }

  if (t == 0) {
    for (int r = rounds; r < 4; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
    res->nInliers = n - nBad; res->nEdges = n; res->rounds = rounds; res->pad = 0;
    poseopt_pose_to_Tcw(est, res->Tcw);
  }
}

}  // namespace

void launch_pose_optimize(hipStream_t s, const PoseOptArgs& a, int nProblems, bool lds) {
  if (nProblems <= 0) return;
  if (lds) hipLaunchKernelGGL(k_pose_optimize<true>, dim3(nProblems), dim3(kPoseOptThreads), 0, s, a);
  else hipLaunchKernelGGL(k_pose_optimize<false>, dim3(nProblems), dim3(kPoseOptThreads), 0, s, a);
}

}  // namespace orbfe
