// initializer_kernels.h -- argument blocks and launchers of the Initializer kernels: the H/F RANSAC (k_initializer.hip,
// arithmetic in initializer_math.h) and ReconstructH / ReconstructF with CheckRT (k_init_reconstruct.hip, arithmetic in
// initializer_reconstruct_math.h).  Host side: initializer.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "initializer_math.h"
#include "initializer_reconstruct_math.h"

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

// k_init_reconstruct.hip: ReconstructH / ReconstructF's hypotheses and CheckRT, one workgroup per (problem, hypothesis)
constexpr int kReconThreads = 256;

struct ReconArgs {
  int nHyp;                   // G: hypotheses in all = workgroups of the launch
  const ReconProblem* probs;
  const int32_t* hypProb;     // [G] problem of hypothesis g
  const float* pairs;         // [N * 4] u1 v1 u2 v2
  const uint32_t* words;      // the problems' inlier words
  uint64_t* keys;             // [slots] scratch: the selection key of every (hypothesis, pair)
  double* R;                  // [G * 9]
  double* t;                  // [G * 3]
  double* cosSel;             // [G]
  double* x3d;                // [slots * 3]
  int32_t* nGood;             // [G]
  int32_t* nInliers;          // [K]
  uint8_t* hypStatus;         // [G]
  uint8_t* pairFlags;         // [slots]
  uint8_t* problemStatus;     // [K]
};

void launch_init_reconstruct(hipStream_t s, const ReconArgs& a);

}  // namespace orbfe
