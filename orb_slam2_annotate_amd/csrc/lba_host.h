// lba_host.h -- the host side of orbfe_local_bundle_adjustment* / orbfe_bundle_adjustment (lba.hip) that needs no device:
// argument checks, the index arrays the kernels read (the edges of a point, the CSR of a free pose's edges, the
// edge_of[pose][point] table, the list of upper blocks of the reduced system), the packing of the staged arrays and the
// schedule of src/Optimizer.cc:689-777 with g2o's Levenberg loop, written over a backend that runs the passes -- the
// kernels in lba.hip, the same work items in a loop in tests/cpp/lba_cpu.cpp.  Plain C++ without a HIP include, so
// tests/cpp/lba_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "lba_math.h"

namespace orbfe {

constexpr int kLbaMaxLocal = 256;       // local key frames of a call: the reduced system is dense, 6 x that wide
constexpr int kLbaMaxPoses = 1 << 16;   // local + fixed
constexpr int kLbaMaxPoints = 1 << 22;
constexpr int kLbaMaxEdges = 1 << 24;
constexpr size_t kLbaMaxTable = (size_t)1 << 24;  // entries of edge_of (free poses x points): 64 MB, rebuilt and uploaded per call

// the operands of a call, as include/orbfe.h names them
struct LbaProblem {
  int nLocal, nFixed;
  const float* Tcw;
  const uint8_t* localIsFixed;
  const float* cam;
  int nPoints;
  const float* xw;  // NULL in the table form: the positions are gathered on the device
  int nEdges;
  const int32_t *edgePose, *edgePoint;
  const float *u, *v, *uRight, *invSigma2;
};

inline bool lba_all_finite(const float* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!(fabsf(p[i]) <= 3.402823466e+38f)) return false;
  return true;
}
inline bool lba_pose_is_free(const LbaProblem& q, int j) { return j < q.nLocal && !(q.localIsFixed && q.localIsFixed[j]); }
inline int lba_count_free(const LbaProblem& q) {
  int n = 0;
  for (int j = 0; j < q.nLocal; j++) n += lba_pose_is_free(q, j);
  return n;
}

// NULL when the operands are fine, else what is wrong with them (one message per check)
inline const char* lba_check(const LbaProblem& q, bool tableForm) {
  if (q.nLocal < 1) return "n_local must be at least 1";
  if (q.nLocal > kLbaMaxLocal) return "more than 256 local key frames";
  if (q.nFixed < 0) return "negative n_fixed";
  if (q.nFixed > kLbaMaxPoses - q.nLocal) return "more than 65536 key frames";
  if (q.nPoints < 1) return "n_points must be at least 1";
  if (q.nPoints > kLbaMaxPoints) return "more than 4194304 points";
  if (q.nEdges < 1) return "n_edges must be at least 1";
  if (q.nEdges > kLbaMaxEdges) return "more than 16777216 edges";
  if (!q.Tcw || !q.cam) return "NULL per-pose array";
  if (!tableForm && !q.xw) return "NULL xw";
  if (!q.edgePose || !q.edgePoint || !q.u || !q.v || !q.uRight || !q.invSigma2) return "NULL per-edge array";
  const int nPoses = q.nLocal + q.nFixed;
  if ((size_t)lba_count_free(q) * (size_t)q.nPoints > kLbaMaxTable) return "free poses x points exceeds 16777216";
  for (int e = 0; e < q.nEdges; e++) {
    if (q.edgePose[e] < 0 || q.edgePose[e] >= nPoses) return "edge_pose out of range";
    if (q.edgePoint[e] < 0 || q.edgePoint[e] >= q.nPoints) return "edge_point out of range";
  }
  for (int e = 1; e < q.nEdges; e++)
    if (q.edgePoint[e] < q.edgePoint[e - 1]) return "edges must be grouped by point: edge_point descends";
  if (!lba_all_finite(q.Tcw, 16 * (size_t)nPoses) || !lba_all_finite(q.cam, 5 * (size_t)nPoses)) return "a pose or camera entry is not finite";
  if (!tableForm && !lba_all_finite(q.xw, 3 * (size_t)q.nPoints)) return "a point coordinate is not finite";
  if (!lba_all_finite(q.u, (size_t)q.nEdges) || !lba_all_finite(q.v, (size_t)q.nEdges) || !lba_all_finite(q.uRight, (size_t)q.nEdges) ||
      !lba_all_finite(q.invSigma2, (size_t)q.nEdges))
    return "an observation is not finite";
  // every point has an edge: the non-decreasing edge_point visits 0 .. n_points - 1 without a gap
  if (q.edgePoint[0] != 0 || q.edgePoint[q.nEdges - 1] != q.nPoints - 1) return "a point without any edge";
  for (int e = 1; e < q.nEdges; e++)
    if (q.edgePoint[e] - q.edgePoint[e - 1] > 1) return "a point without any edge";
  uint8_t seen[kLbaMaxLocal] = {0};
  for (int e = 0; e < q.nEdges; e++)
    if (q.edgePose[e] < q.nLocal) seen[q.edgePose[e]] = 1;
  for (int j = 0; j < q.nLocal; j++)
    if (lba_pose_is_free(q, j) && !seen[j]) return "a free pose without any edge";
  // a key frame observes a point once (MapPoint::mObservations is a map): the edges of a point go to different poses
  for (int e = 0; e < q.nEdges; e++)
    for (int k = e + 1; k < q.nEdges && q.edgePoint[k] == q.edgePoint[e]; k++)
      if (q.edgePose[k] == q.edgePose[e]) return "two edges join the same pose and point";
  return nullptr;
}

// ---- the index arrays ----
inline void lba_fill_free_of(int32_t* freeOf, const LbaProblem& q) {
  int f = 0;
  for (int j = 0; j < q.nLocal + q.nFixed; j++) freeOf[j] = lba_pose_is_free(q, j) ? f++ : -1;
}
inline void lba_fill_pt_off(int32_t* ptOff, const LbaProblem& q) {  // [nPoints + 1]
  int e = 0;
  for (int p = 0; p <= q.nPoints; p++) {
    while (e < q.nEdges && q.edgePoint[e] < p) e++;
    ptOff[p] = e;
  }
}
// a free pose is local: its index f through a table on the stack, so that the fills below need no array another fill made
inline int lba_local_free_of(const LbaProblem& q, int32_t t[kLbaMaxLocal]) {
  int f = 0;
  for (int j = 0; j < q.nLocal; j++) t[j] = lba_pose_is_free(q, j) ? f++ : -1;
  return f;
}
inline int lba_edge_free(const LbaProblem& q, const int32_t* t, int e) { return q.edgePose[e] < q.nLocal ? t[q.edgePose[e]] : -1; }
inline int lba_count_free_edges(const LbaProblem& q) {
  int n = 0;
  for (int e = 0; e < q.nEdges; e++) n += lba_pose_is_free(q, q.edgePose[e]);
  return n;
}
// poseOff [nFree + 1]: the CSR of the free poses' edges
inline void lba_fill_pose_off(int32_t* poseOff, const LbaProblem& q) {
  int32_t t[kLbaMaxLocal];
  const int nFree = lba_local_free_of(q, t);
  for (int f = 0; f <= nFree; f++) poseOff[f] = 0;
  for (int e = 0; e < q.nEdges; e++) {
    const int f = lba_edge_free(q, t, e);
    if (f >= 0) poseOff[f + 1]++;
  }
  for (int f = 0; f < nFree; f++) poseOff[f + 1] += poseOff[f];
}
// poseEdge [lba_count_free_edges]: ascending edge id within a pose
inline void lba_fill_pose_edge(int32_t* poseEdge, const LbaProblem& q) {
  int32_t t[kLbaMaxLocal], cursor[kLbaMaxLocal + 1];
  lba_local_free_of(q, t);
  lba_fill_pose_off(cursor, q);
  for (int e = 0; e < q.nEdges; e++) {
    const int f = lba_edge_free(q, t, e);
    if (f >= 0) poseEdge[cursor[f]++] = e;
  }
}
// edgeOf [nFree][nPoints]
inline void lba_fill_edge_of(int32_t* edgeOf, const LbaProblem& q) {
  int32_t t[kLbaMaxLocal];
  const int nFree = lba_local_free_of(q, t);
  const size_t n = (size_t)nFree * (size_t)q.nPoints;
  for (size_t i = 0; i < n; i++) edgeOf[i] = -1;
  for (int e = 0; e < q.nEdges; e++) {
    const int f = lba_edge_free(q, t, e);
    if (f >= 0) edgeOf[(size_t)f * q.nPoints + q.edgePoint[e]] = e;
  }
}
inline int lba_count_blocks(int nFree) { return nFree * (nFree + 1) / 2; }
inline void lba_fill_blocks(int32_t* blockPose, int nFree) {
  int k = 0;
  for (int i1 = 0; i1 < nFree; i1++)
    for (int i2 = i1; i2 < nFree; i2++, k++) { blockPose[2 * k] = i1; blockPose[2 * k + 1] = i2; }
}

// ---- the staged arrays ----
inline void lba_pack_cam(float* cam8, const LbaProblem& q) {
  for (int j = 0; j < q.nLocal + q.nFixed; j++) {
    for (int k = 0; k < 5; k++) cam8[8 * (size_t)j + k] = q.cam[5 * (size_t)j + k];
    for (int k = 5; k < 8; k++) cam8[8 * (size_t)j + k] = 0.0f;
  }
}
inline void lba_pack_obs(float* obs4, const LbaProblem& q) {
  for (int e = 0; e < q.nEdges; e++) {
    obs4[4 * (size_t)e] = q.u[e]; obs4[4 * (size_t)e + 1] = q.v[e]; obs4[4 * (size_t)e + 2] = q.uRight[e]; obs4[4 * (size_t)e + 3] = q.invSigma2[e];
  }
}
inline void lba_pack_poses(double* pose8, const LbaProblem& q) {  // one estimate buffer: [nPoses][8]
  for (int j = 0; j < q.nLocal + q.nFixed; j++) lba_pose_from_Tcw(q.Tcw + 16 * (size_t)j, pose8 + 8 * (size_t)j);
}
inline void lba_pack_points(double* pt3, const LbaProblem& q) {
  for (size_t i = 0; i < 3 * (size_t)q.nPoints; i++) pt3[i] = (double)q.xw[i];
}

// ---- the schedule ----
struct LbaRun {
  int32_t rounds, stopped, syncs, nLevel1;
  int32_t iterations[2], trials[2], end[2];
  double lambda[2], chi2[2];
};

// One optimize(maxIt) call of SparseOptimizer with the Levenberg algorithm (sparse_optimizer.cpp: terminate() before every
// iteration; optimization_algorithm_levenberg.cpp:102-149: and inside the trial loop).  B: linearise(robust, &rec),
// trial(lambda, robust, &rec), accept() -- 0 or an error code.
template <typename B, typename Stop>
int lba_optimize(B& be, Stop&& stop, int maxIt, bool robust, int rnd, LbaRun* run) {
  LbaLM lm;
  lba_lm_begin(&lm, maxIt);
  LbaRecord rec;
  bool more = maxIt > 0;
  if (!more) lm.end = kLbaEndIterations;
  while (more) {
    if (stop()) { lm.end = kLbaEndStop; break; }
    if (int rc = be.linearise(robust, &rec)) return rc;
    run->syncs++;
    if (rec.nActive == 0) break;  // _ivMap is empty: optimize() returns at once
    lba_lm_after_linearise(&lm, rec);
    do {
      if (int rc = be.trial(lm.lam, robust, &rec)) return rc;
      run->syncs++;
      if (lba_lm_after_trial(&lm, rec)) be.accept();
    } while (lba_lm_more_trials(lm) && !stop());
    more = lba_lm_after_iteration(&lm);
  }
  run->iterations[rnd] = lm.it; run->trials[rnd] = lm.trials; run->end[rnd] = lm.end;
  run->lambda[rnd] = lm.lam; run->chi2[rnd] = lm.cur;
  run->rounds = rnd + 1;
  return 0;
}

// Optimizer::LocalBundleAdjustment from :689 on.  Returns 0 or the backend's error; run->stopped = 1 and nothing done when
// the flag is up at :689.  B also has classify(final): 0 or an error code.
template <typename B, typename Stop>
int lba_schedule_local(B& be, Stop&& stop, LbaRun* run) {
  *run = LbaRun{};
  if (stop()) { run->stopped = 1; return 0; }  // :689-691
  if (int rc = lba_optimize(be, stop, 5, true, 0, run)) return rc;  // :693-694
  if (!stop()) {                                                    // bDoMore (:696-700)
    if (int rc = be.classify(false)) return rc;                     // :705-736
    if (int rc = lba_optimize(be, stop, 10, false, 1, run)) return rc;  // :740-741
  } else {
    run->stopped = 1;
  }
  return be.classify(true);  // :745-777
}
// Optimizer::BundleAdjustment (:54-253): one optimize(nIterations), no classification
template <typename B, typename Stop>
int lba_schedule_global(B& be, Stop&& stop, int nIterations, bool robust, LbaRun* run) {
  *run = LbaRun{};
  const int rc = lba_optimize(be, stop, nIterations, robust, 0, run);
  if (run->end[0] == kLbaEndStop) run->stopped = 1;
  return rc;
}

}  // namespace orbfe
