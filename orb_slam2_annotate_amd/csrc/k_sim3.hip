// k_sim3.hip -- every RANSAC hypothesis of every candidate's Sim3Solver (src/Sim3Solver.cc:173-193: ComputeSim3 on three
// pairs, then CheckInliers over all pairs of the candidate) as one launch: one WAVE per hypothesis, four per workgroup.  All
// 64 lanes run the Horn solve of sim3_math.h on the same three pairs -- wave-uniform, so it costs what one lane would and
// needs neither a broadcast nor LDS -- then lane l tests pairs l, l + 64, ... of the candidate.  Each trip's __ballot is
// stored by lanes 0 and 1 as two uint32 mask words (pair i at bit i & 31 of word i >> 5); the count is the sum of the
// ballots' popcounts.  No atomics, no LDS, no scratch: the 4 x 4 Jacobi is fully unrolled on compile-time indices.  Every
// output byte is a function of the hypothesis's inputs alone, so two runs give identical bytes.
#include <hip/hip_runtime.h>

#include "sim3_kernels.h"

namespace orbfe {

namespace {

__global__ __launch_bounds__(kSim3Threads) void k_sim3(Sim3Args A) {
  const int lane = (int)(threadIdx.x & 63);
  const int h = (int)blockIdx.x * kSim3WavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (h >= A.nHyp) return;  // (a whole wave)
  const Sim3Candidate C = A.cands[A.hypCand[h]];
  float P1[3][3], P2[3][3];
#pragma unroll
  for (int j = 0; j < 3; j++) {
    const size_t p = (size_t)(C.pair0 + A.triples[3 * (size_t)h + j]) * 3;
#pragma unroll
    for (int i = 0; i < 3; i++) { P1[j][i] = A.x3dc1[p + i]; P2[j][i] = A.x3dc2[p + i]; }
  }
  Sim3Transform T;
  sim3_compute(P1, P2, A.fixScale != 0, &T);
  const bool bad = sim3_nonfinite(T);

  uint32_t* words = A.words + (size_t)C.word0 + (size_t)(h - C.hyp0) * (size_t)C.words;
  int count = 0;
  for (int base = 0; base < C.nPairs; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (!bad && i < C.nPairs) {
      const size_t p = (size_t)(C.pair0 + i);
      const float X1[3] = {A.x3dc1[3 * p], A.x3dc1[3 * p + 1], A.x3dc1[3 * p + 2]};
      const float X2[3] = {A.x3dc2[3 * p], A.x3dc2[3 * p + 1], A.x3dc2[3 * p + 2]};
      in = sim3_is_inlier(T, C.K1, C.K2, X1, X2, A.maxErr1[p], A.maxErr2[p]);
    }
    const unsigned long long m = __ballot(in);
    count += __popcll(m);
    const int w = (base >> 5) + lane;  // lanes 0, 1: the two words of this trip
    if (lane < 2 && w < C.words) words[w] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
  }
  if (lane == 0) {
    A.nInliers[h] = count;
    A.status[h] = (uint8_t)(bad ? kSim3Nonfinite : kSim3Ok);
    float* o = A.sim3 + 13 * (size_t)h;  // R, t, s: the binary64 values rounded once (compile-time indices: no scratch)
#pragma unroll
    for (int i = 0; i < 9; i++) o[i] = (float)T.R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) o[9 + i] = (float)T.t[i];
    o[12] = (float)T.s;
  }
}

}  // namespace

void launch_sim3(hipStream_t s, const Sim3Args& a) {
  if (a.nHyp <= 0) return;
  const int blocks = (a.nHyp + kSim3WavesPerBlock - 1) / kSim3WavesPerBlock;
  hipLaunchKernelGGL(k_sim3, dim3(blocks), dim3(kSim3Threads), 0, s, a);
}

}  // namespace orbfe
