// sim3_kernels.h -- argument block and launcher of the Sim3 RANSAC kernel (k_sim3.hip; host side: sim3.hip).  The
// per-hypothesis arithmetic is sim3_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "sim3_math.h"

namespace orbfe {

constexpr int kSim3Threads = 256;  // four waves: one wave per hypothesis
constexpr int kSim3WavesPerBlock = kSim3Threads / 64;

struct Sim3Args {
  int nHyp;
  int fixScale;
  const Sim3Candidate* cands;
  const int32_t* hypCand;   // [nHyp] candidate of hypothesis h
  const int32_t* triples;   // [nHyp * 3] pair indices local to the candidate
  const float *x3dc1, *x3dc2;      // [N * 3]
  const float *maxErr1, *maxErr2;  // [N]
  int32_t* nInliers;   // [nHyp]
  float* sim3;         // [nHyp * 13] R row-major, t, s
  uint32_t* words;     // [sum over candidates of H_k * words_k]
  uint8_t* status;     // [nHyp]
};

void launch_sim3(hipStream_t s, const Sim3Args& a);

}  // namespace orbfe
