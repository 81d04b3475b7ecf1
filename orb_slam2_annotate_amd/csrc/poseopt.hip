// poseopt.hip -- C-ABI entry points of the pose-only optimisation (include/orbfe.h, "Optimizer::PoseOptimization").  A call
// is one staged copy up, ONE launch of k_pose_optimize (k_poseopt.hip) and one copy back on the calling thread's matcher
// stream (arena.h: arena_stage), complete on return.  The argument checks and the interleaving of the edges are
// poseopt_host.h (no device needed).
#include <hip/hip_runtime.h>

#include <algorithm>
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

PoseOptArgs args_begin() {
  PoseOptArgs a{};
  a.deltaMono = (float)std::sqrt(5.991);    // const float deltaMono = sqrt(5.991) (src/Optimizer.cc:291)
  a.deltaStereo = (float)std::sqrt(7.815);  // :292
  return a;
}

hipError_t up_problems(Arena* ar, PoseOptArgs* a, int Q, const int32_t* offsets, const float* K5, const float* Tcw_in) {
  PoseOptProblem* dp;
  TRY(up_pack(ar, &dp, (size_t)Q, [&](PoseOptProblem* hp) {
    for (int p = 0; p < Q; p++) {
      hp[p].off = offsets[p];
      hp[p].n = offsets[p + 1] - offsets[p];
      std::memcpy(hp[p].K5, K5 + 5 * (size_t)p, sizeof hp[p].K5);
      std::memcpy(hp[p].Tcw, Tcw_in + 16 * (size_t)p, sizeof hp[p].Tcw);
      hp[p].pad = 0.0f;
    }
  }));
  a->prob = dp;
  return hipSuccess;
}

int run_batch(int device, int Q, const int32_t* offsets, const float* xw, const float* u, const float* v, const float* u_right,
              const float* inv_sigma2, const float* K5, const float* Tcw_in, float* Tcw_out, uint8_t* outlier,
              int32_t* n_inliers, orbfe_poseopt_stats* stats, double* edge_chi2) {
  if (Q == 0) return ORBFE_OK;
  const int N = offsets[Q];
  const size_t n1 = (size_t)(N ? N : 1);
  int maxN = 0;
  for (int p = 0; p < Q; p++) maxN = std::max(maxN, offsets[p + 1] - offsets[p]);
  PoseOptArgs A = args_begin();
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up_problems(a, &A, Q, offsets, K5, Tcw_in));
    TRY(up_pack(a, &A.edgeA, (size_t)N, [&](float4* h) { poseopt_pack_edges_a(&h->x, N, xw, inv_sigma2); }));
    TRY(up_pack(a, &A.edgeB, (size_t)N, [&](float4* h) { poseopt_pack_edges_b(&h->x, N, u, v, u_right); }));
    open_span(a);  // the three outputs adjacent: one copy back
    A.res = carve<PoseOptResult>(a, (size_t)Q);
    A.level = carve<uint8_t>(a, n1);
    A.chi2 = carve<double>(a, n1);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_pose_optimize(ar->stream, A, Q, maxN <= kPoseOptLdsEdges);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const PoseOptResult* hr = mirror_of(ar, A.res);
  const uint8_t* hl = mirror_of(ar, A.level);
  const double* hc = mirror_of(ar, A.chi2);
  for (int p = 0; p < Q; p++) {
    std::memcpy(Tcw_out + 16 * (size_t)p, hr[p].Tcw, 16 * sizeof(float));
    n_inliers[p] = hr[p].nInliers;
    if (stats) fill_stats(hr[p], stats + p);
    const int off = offsets[p], n = offsets[p + 1] - off;
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
  const size_t n1 = (size_t)(nf ? nf : 1);
  const int32_t offsets[2] = {0, nf};
  PoseOptArgs A = args_begin();
  A.gather = 1;
  A.table = *lock.table;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up_problems(a, &A, 1, offsets, K5, Tcw_in));
    int32_t *ds, *dm, *doct;
    float *dx, *dy, *dur = nullptr, *dlv;  // dur NULL: a monocular frame
    TRY(up(a, &ds, slot, (size_t)n_slots));
    TRY(up(a, &dm, match, (size_t)nf));
    TRY(up(a, &dx, F->x, (size_t)nf));
    TRY(up(a, &dy, F->y, (size_t)nf));
    if (F->u_right) TRY(up(a, &dur, F->u_right, (size_t)nf));
    TRY(up(a, &doct, F->octave, (size_t)nf));
    TRY(up(a, &dlv, inv_level_sigma2, (size_t)n_levels));
    A.edgeA = carve<float4>(a, n1);  // the kernel writes the edges itself: they never travel
    A.edgeB = carve<float4>(a, n1);
    open_span(a);  // the four outputs adjacent: one copy back
    A.res = carve<PoseOptResult>(a, 1);
    A.level = carve<uint8_t>(a, n1);
    A.chi2 = carve<double>(a, n1);
    A.edgeFeat = carve<int32_t>(a, n1);
    A.slot = ds; A.match = dm; A.featX = dx; A.featY = dy; A.featUr = dur; A.featOctave = doct; A.invLevelSigma2 = dlv;
    return close_span(a);
  };
  HIPCHK(arena_stage(lock.device, &ar, stage));
  HIPCHK(flush(ar));
  launch_pose_optimize(ar->stream, A, 1, nf <= kPoseOptLdsEdges);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const PoseOptResult* hr = mirror_of(ar, A.res);
  std::memcpy(Tcw_out, hr->Tcw, 16 * sizeof(float));
  *n_inliers = hr->nInliers;
  if (stats) fill_stats(*hr, stats);
  if (hr->nEdges < 3) return ORBFE_OK;
  const uint8_t* hl = mirror_of(ar, A.level);
  const double* hc = mirror_of(ar, A.chi2);
  const int32_t* hf = mirror_of(ar, A.edgeFeat);
  for (int e = 0; e < hr->nEdges; e++) {  // features without an edge keep their flag (src/Optimizer.cc:301-304)
    outlier[hf[e]] = hl[e];
    if (edge_chi2) edge_chi2[hf[e]] = hc[e];
  }
  return ORBFE_OK;
}
