// poseopt_host.h -- the host side of orbfe_pose_optimization* (poseopt.hip) that needs no device: argument checks and the
// layout of a call in the calling thread's arena.  Plain C++ without a HIP include, so tests/cpp/poseopt_host_san.cpp runs
// exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace orbfe {

constexpr int kPoseOptHostMaxEdges = 16384;      // the frame limit of include/orbfe.h
constexpr int kPoseOptHostMaxProblems = 1 << 20;

inline size_t po_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// A call in the arena: everything below `upEnd` travels up in one copy, [downBegin, total) comes back in one copy.
struct PoseOptLayout {
  size_t oProb, oEdgeA, oEdgeB, oSlot, oMatch, oFeatX, oFeatY, oFeatUr, oFeatOct, oLevelTab, upEnd;
  size_t downBegin, oRes, oLevel, oChi2, oEdgeFeat, total;
};
// Q problems of N edges in all; table form: N = features of the frame, nSlots entries of slot[], nLevels of the level table.
// sizeofProblem / sizeofResult: of the kernel's records (poseopt_kernels.h)
inline PoseOptLayout poseopt_layout(int Q, int N, bool table, bool stereoFrame, int nSlots, int nLevels, size_t sizeofProblem,
                                    size_t sizeofResult) {
  const size_t q = (size_t)(Q > 0 ? Q : 1), n = (size_t)(N > 0 ? N : 1);
  PoseOptLayout L{};
  size_t o = 0;
  L.oProb = o; o += po_align(q * sizeofProblem);
  if (!table) {  // the edges travel
    L.oEdgeA = o; o += po_align(n * 16);
    L.oEdgeB = o; o += po_align(n * 16);
  } else {
    L.oSlot = o; o += po_align((size_t)(nSlots > 0 ? nSlots : 1) * 4);
    L.oMatch = o; o += po_align(n * 4);
    L.oFeatX = o; o += po_align(n * 4);
    L.oFeatY = o; o += po_align(n * 4);
    L.oFeatUr = o; o += stereoFrame ? po_align(n * 4) : 0;
    L.oFeatOct = o; o += po_align(n * 4);
    L.oLevelTab = o; o += po_align((size_t)(nLevels > 0 ? nLevels : 1) * 4);
  }
  L.upEnd = o;
  if (table) {  // the kernel writes the edges itself
    L.oEdgeA = o; o += po_align(n * 16);
    L.oEdgeB = o; o += po_align(n * 16);
  }
  L.downBegin = o;
  L.oRes = o; o += po_align(q * sizeofResult);
  L.oLevel = o; o += po_align(n);
  L.oChi2 = o; o += po_align(n * 8);
  L.oEdgeFeat = o; o += table ? po_align(n * 4) : 0;
  L.total = o;
  return L;
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
