// poseopt.hip -- C-ABI entry points of the pose-only optimisation (include/orbfe.h, "Optimizer::PoseOptimization").  A call
// is one staged copy up, ONE launch of k_pose_optimize (k_poseopt.hip) and one copy back on the calling thread's matcher
// stream (arena.h: arena_scratch), complete on return.  The argument checks and the arena layout are poseopt_host.h (no device
// needed).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "poseopt_host.h"
#include "poseopt_kernels.h"

using namespace orbfe;

namespace {

static_assert(kPoseOptHostMaxEdges == kPoseOptMaxEdges, "one frame limit");

void fill_stats(const PoseOptResult& r, orbfe_poseopt_stats* st) {
  st->rounds = r.rounds;
  for (int k = 0; k < 4; k++) {
    st->iterations[k] = r.iterations[k]; st->trials[k] = r.trials[k];
    st->lambda[k] = r.lambda[k]; st->chi2[k] = r.chi2[k];
  }
}

// what a call leaves in the arena
struct Staged {
  uint8_t *d = nullptr, *h = nullptr;
  hipStream_t s = nullptr;
  PoseOptLayout L{};
  PoseOptArgs a{};
};

int stage_begin(int device, const PoseOptLayout& L, Staged* S) {
  S->L = L;
  Arena* ar;
  HIPCHK(arena_scratch(device, L.total, &ar));
  S->d = ar->base; S->h = ar->hmirror; S->s = ar->stream;
  PoseOptArgs& a = S->a;
  uint8_t* d = S->d;
  a.prob = reinterpret_cast<const PoseOptProblem*>(d + L.oProb);
  a.res = reinterpret_cast<PoseOptResult*>(d + L.oRes);
  a.edgeA = reinterpret_cast<float4*>(d + L.oEdgeA);
  a.edgeB = reinterpret_cast<float4*>(d + L.oEdgeB);
  a.level = d + L.oLevel;
  a.chi2 = reinterpret_cast<double*>(d + L.oChi2);
  a.deltaMono = (float)std::sqrt(5.991);    // const float deltaMono = sqrt(5.991) (src/Optimizer.cc:291)
  a.deltaStereo = (float)std::sqrt(7.815);  // :292
  return ORBFE_OK;
}

// one copy up, the launch, one copy back; the results are in the pinned mirror on return
int stage_run(Staged* S, int Q, bool lds) {
  const PoseOptLayout& L = S->L;
  HIPCHK(hipMemcpyAsync(S->d, S->h, L.upEnd, hipMemcpyHostToDevice, S->s));
  launch_pose_optimize(S->s, S->a, Q, lds);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(S->h + L.downBegin, S->d + L.downBegin, L.total - L.downBegin, hipMemcpyDeviceToHost, S->s));
  HIPCHK(hipStreamSynchronize(S->s));
  return ORBFE_OK;
}

int run_batch(int device, int Q, const int32_t* offsets, const float* xw, const float* u, const float* v, const float* u_right,
              const float* inv_sigma2, const float* K5, const float* Tcw_in, float* Tcw_out, uint8_t* outlier,
              int32_t* n_inliers, orbfe_poseopt_stats* stats, double* edge_chi2) {
  if (Q == 0) return ORBFE_OK;
  const int N = offsets[Q];
  Staged S;
  int rc = stage_begin(device, poseopt_layout(Q, N, false, false, 0, 0, sizeof(PoseOptProblem), sizeof(PoseOptResult)), &S);
  if (rc) return rc;
  const PoseOptLayout& L = S.L;
  PoseOptProblem* hp = reinterpret_cast<PoseOptProblem*>(S.h + L.oProb);
  int maxN = 0;
  for (int p = 0; p < Q; p++) {
    hp[p].off = offsets[p];
    hp[p].n = offsets[p + 1] - offsets[p];
    if (hp[p].n > maxN) maxN = hp[p].n;
    std::memcpy(hp[p].K5, K5 + 5 * (size_t)p, sizeof hp[p].K5);
    std::memcpy(hp[p].Tcw, Tcw_in + 16 * (size_t)p, sizeof hp[p].Tcw);
    hp[p].pad = 0.0f;
  }
  float* hA = reinterpret_cast<float*>(S.h + L.oEdgeA);
  float* hB = reinterpret_cast<float*>(S.h + L.oEdgeB);
  for (int i = 0; i < N; i++) {
    hA[4 * i] = xw[3 * i]; hA[4 * i + 1] = xw[3 * i + 1]; hA[4 * i + 2] = xw[3 * i + 2]; hA[4 * i + 3] = inv_sigma2[i];
    hB[4 * i] = u[i]; hB[4 * i + 1] = v[i]; hB[4 * i + 2] = u_right[i]; hB[4 * i + 3] = 0.0f;
  }
  S.a.gather = 0;
  rc = stage_run(&S, Q, maxN <= kPoseOptLdsEdges);
  if (rc) return rc;
  const PoseOptResult* hr = reinterpret_cast<const PoseOptResult*>(S.h + L.oRes);
  const uint8_t* hl = S.h + L.oLevel;
  const double* hc = reinterpret_cast<const double*>(S.h + L.oChi2);
  for (int p = 0; p < Q; p++) {
    std::memcpy(Tcw_out + 16 * (size_t)p, hr[p].Tcw, 16 * sizeof(float));
    n_inliers[p] = hr[p].nInliers;
    if (stats) fill_stats(hr[p], stats + p);
    const int n = hp[p].n, off = hp[p].off;
    if (n < 3) continue;  // pose and flags untouched (src/Optimizer.cc:385)
    std::memcpy(outlier + off, hl + off, (size_t)n);
    if (edge_chi2) std::memcpy(edge_chi2 + off, hc + off, (size_t)n * sizeof(double));
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_pose_optimization_batch(int device, int n_problems, const int32_t* offsets, const float* xw, const float* u,
                                             const float* v, const float* u_right, const float* inv_sigma2, const float* K5,
                                             const float* Tcw_in, float* Tcw_out, uint8_t* outlier, int32_t* n_inliers,
                                             orbfe_poseopt_stats* stats, double* edge_chi2) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, "pose_optimization_batch: negative device");
  if (const char* e = poseopt_check_batch(n_problems, offsets, xw, u, v, u_right, inv_sigma2, K5, Tcw_in, Tcw_out, outlier, n_inliers))
    return fail(ORBFE_ERR_INVALID, std::string("pose_optimization_batch: ") + e);
  return run_batch(device, n_problems, offsets, xw, u, v, u_right, inv_sigma2, K5, Tcw_in, Tcw_out, outlier, n_inliers, stats,
                   edge_chi2);
}

extern "C" int orbfe_pose_optimization(int device, int n, const float* xw, const float* u, const float* v, const float* u_right,
                                       const float* inv_sigma2, const float* K5, const float* Tcw_in, float* Tcw_out,
                                       uint8_t* outlier, int32_t* n_inliers, orbfe_poseopt_stats* stats, double* edge_chi2) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, "pose_optimization: negative device");
  if (const char* e = poseopt_check_single(n, xw, u, v, u_right, inv_sigma2, K5, Tcw_in, Tcw_out, outlier, n_inliers))
    return fail(ORBFE_ERR_INVALID, std::string("pose_optimization: ") + e);
  const int32_t offsets[2] = {0, n};
  return run_batch(device, 1, offsets, xw, u, v, u_right, inv_sigma2, K5, Tcw_in, Tcw_out, outlier, n_inliers, stats, edge_chi2);
}

extern "C" int orbfe_pose_optimization_mappoints(orbfe_mappoints* mp, int n_slots, const int32_t* slot, const orbfe_frame_view* F,
                                                 const int32_t* match, const float* inv_level_sigma2, int n_levels,
                                                 const float* K5, const float* Tcw_in, float* Tcw_out, uint8_t* outlier,
                                                 int32_t* n_inliers, orbfe_poseopt_stats* stats, double* edge_chi2) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "pose_optimization_mappoints: NULL table");
  if (!F) return fail(ORBFE_ERR_INVALID, "pose_optimization_mappoints: NULL frame");
  if (F->resident) F = orbfe_frame_get_view(F->resident);  // (the handle's own host copies)
  if (const char* e = poseopt_check_table(orbfe_mappoints_capacity(mp), n_slots, slot, F->n, match, F->octave, F->x, F->y,
                                          inv_level_sigma2, n_levels, K5, Tcw_in, Tcw_out, outlier, n_inliers))
    return fail(ORBFE_ERR_INVALID, std::string("pose_optimization_mappoints: ") + e);
  const int nf = F->n;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  Staged S;
  int rc = stage_begin(lock.device, poseopt_layout(1, nf, true, F->u_right != nullptr, n_slots, n_levels, sizeof(PoseOptProblem),
                                                   sizeof(PoseOptResult)), &S);
  if (rc) return rc;
  const PoseOptLayout& L = S.L;
  PoseOptProblem* hp = reinterpret_cast<PoseOptProblem*>(S.h + L.oProb);
  hp->off = 0; hp->n = nf; hp->pad = 0.0f;
  std::memcpy(hp->K5, K5, sizeof hp->K5);
  std::memcpy(hp->Tcw, Tcw_in, sizeof hp->Tcw);
  if (n_slots) std::memcpy(S.h + L.oSlot, slot, (size_t)n_slots * 4);
  if (nf) {
    std::memcpy(S.h + L.oMatch, match, (size_t)nf * 4);
    std::memcpy(S.h + L.oFeatX, F->x, (size_t)nf * 4);
    std::memcpy(S.h + L.oFeatY, F->y, (size_t)nf * 4);
    if (F->u_right) std::memcpy(S.h + L.oFeatUr, F->u_right, (size_t)nf * 4);
    std::memcpy(S.h + L.oFeatOct, F->octave, (size_t)nf * 4);
  }
  std::memcpy(S.h + L.oLevelTab, inv_level_sigma2, (size_t)n_levels * 4);
  PoseOptArgs& a = S.a;
  a.gather = 1;
  a.table = *lock.table;
  a.slot = reinterpret_cast<const int32_t*>(S.d + L.oSlot);
  a.match = reinterpret_cast<const int32_t*>(S.d + L.oMatch);
  a.featX = reinterpret_cast<const float*>(S.d + L.oFeatX);
  a.featY = reinterpret_cast<const float*>(S.d + L.oFeatY);
  a.featUr = F->u_right ? reinterpret_cast<const float*>(S.d + L.oFeatUr) : nullptr;
  a.featOctave = reinterpret_cast<const int32_t*>(S.d + L.oFeatOct);
  a.invLevelSigma2 = reinterpret_cast<const float*>(S.d + L.oLevelTab);
  a.edgeFeat = reinterpret_cast<int32_t*>(S.d + L.oEdgeFeat);
  rc = stage_run(&S, 1, nf <= kPoseOptLdsEdges);
  if (rc) return rc;
  const PoseOptResult* hr = reinterpret_cast<const PoseOptResult*>(S.h + L.oRes);
  std::memcpy(Tcw_out, hr->Tcw, 16 * sizeof(float));
  *n_inliers = hr->nInliers;
  if (stats) fill_stats(*hr, stats);
  if (hr->nEdges < 3) return ORBFE_OK;
  const uint8_t* hl = S.h + L.oLevel;
  const double* hc = reinterpret_cast<const double*>(S.h + L.oChi2);
  const int32_t* hf = reinterpret_cast<const int32_t*>(S.h + L.oEdgeFeat);
  for (int e = 0; e < hr->nEdges; e++) {  // features without an edge keep their flag (src/Optimizer.cc:301-304)
    outlier[hf[e]] = hl[e];
    if (edge_chi2) edge_chi2[hf[e]] = hc[e];
  }
  return ORBFE_OK;
}
