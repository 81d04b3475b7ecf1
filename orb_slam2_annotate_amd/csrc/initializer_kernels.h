// initializer_kernels.h -- argument block and launcher of the Initializer H/F RANSAC kernel (k_initializer.hip; host side:
// initializer.hip).  The per-hypothesis arithmetic is initializer_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "initializer_math.h"

namespace orbfe {

constexpr int kInitThreads = 256;  // four waves: one wave per (set, model)
constexpr int kInitWavesPerBlock = kInitThreads / 64;

struct InitArgs {
  int nHyp;                   // sets in all; the launch has 2 nHyp waves, wave 2 h + model
  const InitProblem* probs;
  const int32_t* hypProb;     // [nHyp] problem of set h
  const int32_t* sets;        // [nHyp * 8] pair indices local to the problem
  const float* pairs;         // [N * 4] u1 v1 u2 v2
  double* score;              // [nHyp * 2]
  double* model;              // [nHyp * 2 * 9] H21 / F21, row-major
  double* h12;                // [nHyp * 9]
  int32_t* nInliers;          // [nHyp * 2]
  uint32_t* words;            // [sum over problems of 2 H_k words_k]
  uint8_t* status;            // [nHyp * 2]
};

void launch_initializer(hipStream_t s, const InitArgs& a);

}  // namespace orbfe
