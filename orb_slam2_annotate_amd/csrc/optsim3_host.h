// optsim3_host.h -- the host side of orbfe_optimize_sim3* (optsim3.hip) that needs no device: argument checks and the packing
// of the per-pair arrays and the per-problem records the kernel reads.  Plain C++ without a HIP include, so
// tests/cpp/optsim3_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers and
// tests/cpp/optsim3_cpu.cpp lays its problems out with it.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "optsim3_math.h"

namespace orbfe {

constexpr int kOptSim3HostMaxPairs = 16384;  // the per-problem limit of include/orbfe.h
constexpr int kOptSim3HostMaxProblems = 1 << 20;

// The N pairs of a call as the kernel reads them (optsim3_kernels.h: OptSim3Args), 4 N floats each: A[4 i ..] = (X1, invSigma2_1),
// B[4 i ..] = (X2, invSigma2_2), C[4 i ..] = (obs1, obs2).  One function per destination: each array is staged on its own
inline void optsim3_pack_pairs_a(float* A, int n, const float* x3dc1, const float* inv_sigma2_1) {
  for (int i = 0; i < n; i++) {
    A[4 * i] = x3dc1[3 * i]; A[4 * i + 1] = x3dc1[3 * i + 1]; A[4 * i + 2] = x3dc1[3 * i + 2]; A[4 * i + 3] = inv_sigma2_1[i];
  }
}
inline void optsim3_pack_pairs_b(float* B, int n, const float* x3dc2, const float* inv_sigma2_2) {
  for (int i = 0; i < n; i++) {
    B[4 * i] = x3dc2[3 * i]; B[4 * i + 1] = x3dc2[3 * i + 1]; B[4 * i + 2] = x3dc2[3 * i + 2]; B[4 * i + 3] = inv_sigma2_2[i];
  }
}
inline void optsim3_pack_pairs_c(float* C, int n, const float* obs1, const float* obs2) {
  for (int i = 0; i < n; i++) {
    C[4 * i] = obs1[2 * i]; C[4 * i + 1] = obs1[2 * i + 1]; C[4 * i + 2] = obs2[2 * i]; C[4 * i + 3] = obs2[2 * i + 1];
  }
}
inline void optsim3_pack_problems(OptSim3Problem* P, int K, const int32_t* pair_off, const float* cam1, const float* cam2,
                                  const float* sim3_in, const float* th2, const uint8_t* fix_scale) {
  for (int p = 0; p < K; p++) {
    P[p].off = pair_off[p];
    P[p].n = pair_off[p + 1] - pair_off[p];
    for (int k = 0; k < 4; k++) { P[p].cam1[k] = cam1[4 * (size_t)p + k]; P[p].cam2[k] = cam2[4 * (size_t)p + k]; }
    for (int k = 0; k < 13; k++) P[p].sim3[k] = sim3_in[13 * (size_t)p + k];
    P[p].th2 = th2[p];
    P[p].delta = sqrtf(th2[p]);  // const float deltaHuber = sqrt(th2) (src/Optimizer.cc:1168)
    P[p].fixScale = fix_scale[p] ? 1 : 0;
  }
}

// NULL when the arguments are fine, else what is wrong with them.  pair_off: K + 1 ascending entries from 0
inline const char* optsim3_check_multi(int K, const int32_t* pair_off, const float* x3dc1, const float* x3dc2, const float* obs1,
                                       const float* obs2, const float* inv_sigma2_1, const float* inv_sigma2_2, const float* cam1,
                                       const float* cam2, const float* sim3_in, const float* th2, const uint8_t* fix_scale,
                                       const double* sim3_out, const uint8_t* bad, const int32_t* n_in) {
  if (K < 0) return "negative problem count";
  if (K > kOptSim3HostMaxProblems) return "more than 1048576 problems";
  if (!pair_off) return "NULL pair_off";
  if (pair_off[0] != 0) return "pair_off[0] must be 0";
  for (int i = 0; i < K; i++) {
    if (pair_off[i + 1] < pair_off[i]) return "pair_off must not descend";
    if (pair_off[i + 1] - pair_off[i] > kOptSim3HostMaxPairs) return "more than 16384 pairs in one problem";
  }
  if (K > 0 && (!cam1 || !cam2 || !sim3_in || !th2 || !fix_scale || !sim3_out || !n_in)) return "NULL per-problem array";
  if (pair_off[K] > 0 && (!x3dc1 || !x3dc2 || !obs1 || !obs2 || !inv_sigma2_1 || !inv_sigma2_2 || !bad)) return "NULL per-pair array";
  for (int i = 0; i < K; i++)
    if (!(th2[i] > 0.0f) || !(th2[i] <= 3.402823466e+38f)) return "th2 must be positive and finite";
  return nullptr;
}

inline const char* optsim3_check_single(int n, const float* x3dc1, const float* x3dc2, const float* obs1, const float* obs2,
                                        const float* inv_sigma2_1, const float* inv_sigma2_2, const float* cam1, const float* cam2,
                                        const float* sim3_in, float th2, const double* sim3_out, const uint8_t* bad,
                                        const int32_t* n_in) {
  if (n < 0) return "negative count";
  if (n > kOptSim3HostMaxPairs) return "more than 16384 pairs";
  const int32_t off[2] = {0, n};
  const uint8_t fix = 0;
  return optsim3_check_multi(1, off, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, &th2, &fix,
                             sim3_out, bad, n_in);
}

}  // namespace orbfe
