// poseopt_host.h -- the host side of orbfe_pose_optimization* (poseopt.hip) that needs no device: argument checks and the
// interleaving of the edge arrays into the kernel's float4 records.  Plain C++ without a HIP include, so
// tests/cpp/poseopt_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace orbfe {

constexpr int kPoseOptHostMaxEdges = 16384;      // the frame limit of include/orbfe.h
constexpr int kPoseOptHostMaxProblems = 1 << 20;

// The n edges of a call as the kernel reads them (poseopt_kernels.h: PoseOptArgs): A[4 i ..] = (Xw.x, Xw.y, Xw.z, inv_sigma2)
// and B[4 i ..] = (u, v, u_right, 0), 4 n floats each.  One function per destination: each array is staged on its own
inline void poseopt_pack_edges_a(float* A, int n, const float* xw, const float* inv_sigma2) {
  for (int i = 0; i < n; i++) {
    A[4 * i] = xw[3 * i]; A[4 * i + 1] = xw[3 * i + 1]; A[4 * i + 2] = xw[3 * i + 2]; A[4 * i + 3] = inv_sigma2[i];
  }
}
inline void poseopt_pack_edges_b(float* B, int n, const float* u, const float* v, const float* u_right) {
  for (int i = 0; i < n; i++) {
    B[4 * i] = u[i]; B[4 * i + 1] = v[i]; B[4 * i + 2] = u_right[i]; B[4 * i + 3] = 0.0f;
  }
}

// NULL when the arguments of the array forms are fine, else what is wrong with them.  offsets: Q + 1 ascending entries from 0
inline const char* poseopt_check_batch(int Q, const int32_t* offsets, const float* xw, const float* u, const float* v,
                                       const float* u_right, const float* inv_sigma2, const float* K5, const float* Tcw_in,
                                       const float* Tcw_out, const uint8_t* outlier, const int32_t* n_inliers) {
  if (Q < 0) return "negative problem count";
  if (Q > kPoseOptHostMaxProblems) return "more than 1048576 problems";
  if (!offsets) return "NULL offsets";
  if (offsets[0] != 0) return "offsets[0] must be 0";
  for (int i = 0; i < Q; i++) {
    if (offsets[i + 1] < offsets[i]) return "offsets must not descend";
    if (offsets[i + 1] - offsets[i] > kPoseOptHostMaxEdges) return "more than 16384 edges in one problem";
  }
  if (Q > 0 && (!K5 || !Tcw_in || !Tcw_out || !n_inliers)) return "NULL array";
  if (offsets[Q] > 0 && (!xw || !u || !v || !u_right || !inv_sigma2 || !outlier)) return "NULL array";
  return nullptr;
}

inline const char* poseopt_check_single(int n, const float* xw, const float* u, const float* v, const float* u_right,
                                        const float* inv_sigma2, const float* K5, const float* Tcw_in, const float* Tcw_out,
                                        const uint8_t* outlier, const int32_t* n_inliers) {
  if (n < 0) return "negative count";
  if (n > kPoseOptHostMaxEdges) return "more than 16384 edges";
  const int32_t offsets[2] = {0, n};
  return poseopt_check_batch(1, offsets, xw, u, v, u_right, inv_sigma2, K5, Tcw_in, Tcw_out, outlier, n_inliers);
}

// the table form: slot[] inside the table, match[] inside slot[], the octave of every matched feature inside the level table
inline const char* poseopt_check_table(int capacity, int n_slots, const int32_t* slot, int nFeat, const int32_t* match,
                                       const int32_t* octave, const float* x, const float* y, const float* inv_level_sigma2,
                                       int n_levels, const float* K5, const float* Tcw_in, const float* Tcw_out,
                                       const uint8_t* outlier, const int32_t* n_inliers) {
  if (n_slots < 0 || nFeat < 0) return "negative count";
  if (nFeat > kPoseOptHostMaxEdges) return "more than 16384 features";
  if (n_slots > 0 && !slot) return "NULL slot list";
  for (int i = 0; i < n_slots; i++)
    if (slot[i] < 0 || slot[i] >= capacity) return "slot outside [0, capacity)";
  if (!inv_level_sigma2 || n_levels <= 0) return "no level table";
  if (!K5 || !Tcw_in || !Tcw_out || !n_inliers) return "NULL array";
  if (nFeat > 0 && (!match || !octave || !x || !y || !outlier)) return "NULL array";
  for (int i = 0; i < nFeat; i++) {
    if (match[i] >= n_slots) return "match outside slot[]";
    if (match[i] >= 0 && (octave[i] < 0 || octave[i] >= n_levels)) return "octave outside the level table";
  }
  return nullptr;
}

}  // namespace orbfe
