// optsim3_kernels.h -- argument block and launcher of the Sim3 optimisation kernel (k_optsim3.hip; host side: optsim3.hip).
// The arithmetic is optsim3_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "optsim3_math.h"

namespace orbfe {

constexpr int kOptSim3Threads = 64;      // one wave per problem: lane l owns pairs l, l + 64, ...
constexpr int kOptSim3MaxPairs = 16384;  // the per-problem limit of include/orbfe.h

struct OptSim3Args {
  const OptSim3Problem* prob;
  OptSim3Result* res;
  const float4* pairA;  // (X1.x, X1.y, X1.z, invSigma2_1) per pair
  const float4* pairB;  // (X2.x, X2.y, X2.z, invSigma2_2)
  const float4* pairC;  // (obs1.x, obs1.y, obs2.x, obs2.y)
  uint8_t* bad;         // per pair: 0 kept, 1 erased after round one, 2 erased after round two
  double* chi12;        // per pair: chi2 of the error g2o would hold in e12 (what the classifications read)
  double* chi21;
};

// one 64-lane workgroup per problem
void launch_optimize_sim3(hipStream_t s, const OptSim3Args& a, int nProblems);

}  // namespace orbfe
