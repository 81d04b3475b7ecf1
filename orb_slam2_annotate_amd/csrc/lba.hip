// lba.hip -- C-ABI entry points of the bundle adjustments (include/orbfe.h, "Optimizer::LocalBundleAdjustment").  A call is
// one staged copy up, then g2o's Levenberg loop on the host (lba_host.h: lba_schedule_*) over the kernels of k_lba.hip on the
// calling thread's matcher stream: per linearisation and per trial one group of launches and one small record back, at the
// end one copy of the results.  Everything lives in the thread's arena (arena.h: arena_stage): no allocation and no event
// of its own.  The argument checks, the index arrays and the packing are lba_host.h (no device needed).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "lba_host.h"
#include "lba_kernels.h"

using namespace orbfe;

namespace {

static_assert(kLbaMaxLocal == kLbaSolveMaxPoses, "one limit on the local key frames");

// the passes on the device, as lba_host.h's schedule calls them
struct DeviceBackend {
  Arena* ar;
  LbaArgs A;
  uint8_t* erase;
  int cur = 0;
  hipError_t err = hipSuccess;

  int record(LbaRecord* r) {
    err = hipGetLastError();
    if (err == hipSuccess) err = down_range(ar, A.rec, A.rec + 1);
    if (err == hipSuccess) err = hipStreamSynchronize(ar->stream);
    if (err != hipSuccess) return 1;
    *r = *mirror_of(ar, A.rec);
    return 0;
  }
  int linearise(bool robust, LbaRecord* r) {
    launch_lba_linearise(ar->stream, A, cur, robust);
    return record(r);
  }
  int trial(double lambda, bool robust, LbaRecord* r) {
    launch_lba_trial(ar->stream, A, cur, lambda, robust);
    return record(r);
  }
  void accept() { cur = 1 - cur; }
  int classify(bool final) {
    launch_lba_classify(ar->stream, A, cur, final, erase);
    err = hipGetLastError();
    return err != hipSuccess;
  }
};

void fill_stats(const LbaRun& run, bool stopped, orbfe_lba_stats* st) {
  if (!st) return;
  st->rounds = run.rounds; st->stopped = stopped; st->host_syncs = run.syncs; st->n_level1 = run.nLevel1;
  for (int r = 0; r < 2; r++) {
    st->iterations[r] = run.iterations[r]; st->trials[r] = run.trials[r]; st->termination[r] = run.end[r];
    st->lambda[r] = run.lambda[r]; st->chi2[r] = run.chi2[r];
  }
}

// mp NULL: the array form.  local false: orbfe_bundle_adjustment
int run(const char* name, int device, orbfe_mappoints* mp, const int32_t* slot, const LbaProblem& q, bool local, int nIterations,
        int robust, const volatile int* stop_flag, double* Tcw_out, double* xw_out, uint8_t* erase, uint8_t* level1,
        orbfe_lba_stats* stats, double* edge_chi2) {
  const std::string pre = std::string(name) + ": ";
  if (const char* e = lba_check(q, mp != nullptr)) return fail(ORBFE_ERR_INVALID, pre + e);
  if (!Tcw_out || (!mp && !xw_out) || (local && !erase)) return fail(ORBFE_ERR_INVALID, pre + "NULL output array");
  if (!local && nIterations < 0) return fail(ORBFE_ERR_INVALID, pre + "negative n_iterations");
  const int nPoses = q.nLocal + q.nFixed, nFree = lba_count_free(q), nFreeEdges = lba_count_free_edges(q);
  const int nBlocks = lba_count_blocks(nFree);
  const size_t nP = (size_t)q.nPoints, nE = (size_t)q.nEdges, n6 = 6 * (size_t)nFree;
  bool seen = false;
  auto stop = [&]() -> bool {
    const bool s = stop_flag && *stop_flag != 0;
    seen = seen || s;
    return s;
  };
  DeviceBackend be{};
  LbaArgs& A = be.A;
  A.nPoses = nPoses; A.nFree = nFree; A.nPoints = q.nPoints; A.nEdges = q.nEdges;
  int32_t* dslot = nullptr;
  auto stage = [&](Arena* a) -> hipError_t {
    float *dcam, *dobs;
    int32_t *dfree, *dep, *dept, *dpo, *dpoff, *dpe, *deo, *dbp;
    uint8_t* dlevel;
    double *dpose, *dchi;
    TRY(up_pack(a, &dcam, 8 * (size_t)nPoses, [&](float* h) { lba_pack_cam(h, q); }));
    TRY(up_pack(a, &dobs, 4 * nE, [&](float* h) { lba_pack_obs(h, q); }));
    TRY(up_pack(a, &dfree, (size_t)nPoses, [&](int32_t* h) { lba_fill_free_of(h, q); }));
    TRY(up(a, &dep, q.edgePose, nE));
    TRY(up(a, &dept, q.edgePoint, nE));
    TRY(up_pack(a, &dpo, nP + 1, [&](int32_t* h) { lba_fill_pt_off(h, q); }));
    TRY(up_pack(a, &dpoff, (size_t)nFree + 1, [&](int32_t* h) { lba_fill_pose_off(h, q); }));
    TRY(up_pack(a, &dpe, (size_t)nFreeEdges, [&](int32_t* h) { lba_fill_pose_edge(h, q); }));
    TRY(up_pack(a, &deo, (size_t)nFree * nP, [&](int32_t* h) { lba_fill_edge_of(h, q); }));
    TRY(up_pack(a, &dbp, 2 * (size_t)nBlocks, [&](int32_t* h) { lba_fill_blocks(h, nFree); }));
    if (mp) TRY(up(a, &dslot, slot, nP));
    TRY(up_fill(a, &dlevel, nE, 0));
    TRY(up_fill(a, &dchi, nE, 0));
    // both estimate buffers start as the converted inputs: a vertex no pass touches reads the same in either
    TRY(up_pack(a, &dpose, 16 * (size_t)nPoses, [&](double* h) {
      lba_pack_poses(h, q);
      lba_pack_poses(h + 8 * (size_t)nPoses, q);
    }));
    if (mp) {
      A.pt = carve<double>(a, 6 * nP);
    } else {
      TRY(up_pack(a, &A.pt, 6 * nP, [&](double* h) {
        lba_pack_points(h, q);
        lba_pack_points(h + 3 * nP, q);
      }));
    }
    A.cam = dcam; A.edgeObs = dobs; A.freeOf = dfree; A.edgePose = dep; A.edgePoint = dept; A.ptOff = dpo; A.poseOff = dpoff;
    A.poseEdge = dpe; A.edgeOf = deo; A.blockPose = dbp; A.level = dlevel; A.chi2 = dchi; A.pose = dpose;
    be.erase = carve<uint8_t>(a, nE);
    A.rec = carve<LbaRecord>(a, 1);
    A.lin = carve<double>(a, kLbaLin * nE);
    A.Y = carve<double>(a, 18 * nE);
    A.Hll = carve<double>(a, 6 * nP); A.bl = carve<double>(a, 3 * nP); A.HllInv = carve<double>(a, 6 * nP); A.Db = carve<double>(a, 3 * nP);
    A.ptRho = carve<double>(a, nP); A.ptScale = carve<double>(a, nP); A.ptAct = carve<uint8_t>(a, nP);
    A.Hpp = carve<double>(a, 21 * (size_t)nFree + 1); A.bp = carve<double>(a, n6 + 1); A.poseScale = carve<double>(a, (size_t)nFree + 1);
    A.poseAct = carve<uint8_t>(a, (size_t)nFree + 1);
    A.S = carve<double>(a, n6 * n6 + 1); A.bs = carve<double>(a, n6 + 1); A.xp = carve<double>(a, n6 + 1);
    // the mirror reaches everything that travels back (level .. rec): the scratch behind it never does
    return a->sizing ? hipSuccess : grow_mirror(a, (size_t)(reinterpret_cast<uint8_t*>(A.rec + 1) - a->base.p));
  };
  LbaRun runStats{};
  if (local && stop()) {  // :689-691: nothing is optimised; the outputs are the converted inputs
    for (int j = 0; j < q.nLocal; j++) {
      double P[8];
      lba_pose_from_Tcw(q.Tcw + 16 * (size_t)j, P);
      lba_pose_to_Tcw(P, Tcw_out + 16 * (size_t)j);
    }
    if (xw_out && !mp) lba_pack_points(xw_out, q);
    std::memset(erase, 0, nE);
    if (level1) std::memset(level1, 0, nE);
    if (edge_chi2) std::memset(edge_chi2, 0, nE * sizeof(double));
    fill_stats(runStats, true, stats);
    return ORBFE_OK;
  }
  if (mp) {
    MapPointsLock lock(mp);
    if (lock.rc) return lock.rc;
    HIPCHK(arena_stage(lock.device, &be.ar, stage));
    HIPCHK(flush(be.ar));
    launch_lba_gather(be.ar->stream, A, *lock.table, dslot);
    // the second estimate buffer starts equal to the first
    HIPCHK(hipMemcpyAsync(A.pt + 3 * nP, A.pt, 3 * nP * sizeof(double), hipMemcpyDeviceToDevice, be.ar->stream));
    const int rc = lba_schedule_local(be, stop, &runStats);
    if (rc) return fail(hip_status(be.err), pre + hipGetErrorString(be.err));
    launch_lba_scatter(be.ar->stream, A, be.cur, *lock.table, dslot);
    HIPCHK(hipGetLastError());
    HIPCHK(down_range(be.ar, A.level, A.rec + 1));
    HIPCHK(hipStreamSynchronize(be.ar->stream));  // (the lock's scope ends behind the scatter)
  } else {
    HIPCHK(arena_stage(device, &be.ar, stage));
    HIPCHK(flush(be.ar));
    const int rc = local ? lba_schedule_local(be, stop, &runStats) : lba_schedule_global(be, stop, nIterations, robust != 0, &runStats);
    if (rc) return fail(hip_status(be.err), pre + hipGetErrorString(be.err));
    HIPCHK(down_range(be.ar, A.level, A.rec + 1));
    HIPCHK(hipStreamSynchronize(be.ar->stream));
  }
  runStats.syncs++;
  const double* hp = mirror_of(be.ar, A.pose) + (size_t)be.cur * 8 * (size_t)nPoses;
  for (int j = 0; j < q.nLocal; j++) lba_pose_to_Tcw(hp + 8 * (size_t)j, Tcw_out + 16 * (size_t)j);
  if (xw_out) std::memcpy(xw_out, mirror_of(be.ar, A.pt) + (size_t)be.cur * 3 * nP, 3 * nP * sizeof(double));
  const uint8_t* hl = mirror_of(be.ar, A.level);
  if (local) {
    std::memcpy(erase, mirror_of(be.ar, be.erase), nE);
    for (size_t e = 0; e < nE; e++) runStats.nLevel1 += hl[e] != 0;
    if (level1) std::memcpy(level1, hl, nE);
  }
  if (edge_chi2) std::memcpy(edge_chi2, mirror_of(be.ar, A.chi2), nE * sizeof(double));
  fill_stats(runStats, seen, stats);
  return ORBFE_OK;
}

LbaProblem problem(int n_local, int n_fixed, const float* Tcw, const uint8_t* local_is_fixed, const float* cam, int n_points,
                   const float* xw, int n_edges, const int32_t* edge_pose, const int32_t* edge_point, const float* u, const float* v,
                   const float* u_right, const float* inv_sigma2) {
  return LbaProblem{n_local, n_fixed, Tcw, local_is_fixed, cam, n_points, xw, n_edges, edge_pose, edge_point, u, v, u_right, inv_sigma2};
}

}  // namespace

extern "C" int orbfe_local_bundle_adjustment(int device, int n_local, int n_fixed, const float* Tcw, const uint8_t* local_is_fixed,
                                             const float* cam, int n_points, const float* xw, int n_edges, const int32_t* edge_pose,
                                             const int32_t* edge_point, const float* u, const float* v, const float* u_right,
                                             const float* inv_sigma2, const volatile int* stop_flag, double* Tcw_out, double* xw_out,
                                             uint8_t* erase, uint8_t* level1, orbfe_lba_stats* stats, double* edge_chi2) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, "local_bundle_adjustment: negative device");
  return run("local_bundle_adjustment", device, nullptr, nullptr,
             problem(n_local, n_fixed, Tcw, local_is_fixed, cam, n_points, xw, n_edges, edge_pose, edge_point, u, v, u_right, inv_sigma2),
             true, 0, 1, stop_flag, Tcw_out, xw_out, erase, level1, stats, edge_chi2);
}

extern "C" int orbfe_bundle_adjustment(int device, int n_local, int n_fixed, const float* Tcw, const uint8_t* local_is_fixed,
                                       const float* cam, int n_points, const float* xw, int n_edges, const int32_t* edge_pose,
                                       const int32_t* edge_point, const float* u, const float* v, const float* u_right,
                                       const float* inv_sigma2, int n_iterations, int robust, const volatile int* stop_flag,
                                       double* Tcw_out, double* xw_out, orbfe_lba_stats* stats, double* edge_chi2) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, "bundle_adjustment: negative device");
  return run("bundle_adjustment", device, nullptr, nullptr,
             problem(n_local, n_fixed, Tcw, local_is_fixed, cam, n_points, xw, n_edges, edge_pose, edge_point, u, v, u_right, inv_sigma2),
             false, n_iterations, robust, stop_flag, Tcw_out, xw_out, nullptr, nullptr, stats, edge_chi2);
}

extern "C" int orbfe_local_bundle_adjustment_mappoints(orbfe_mappoints* mp, int n_points, const int32_t* slot, int n_local, int n_fixed,
                                                       const float* Tcw, const uint8_t* local_is_fixed, const float* cam, int n_edges,
                                                       const int32_t* edge_pose, const int32_t* edge_point, const float* u,
                                                       const float* v, const float* u_right, const float* inv_sigma2,
                                                       const volatile int* stop_flag, double* Tcw_out, double* xw_out, uint8_t* erase,
                                                       uint8_t* level1, orbfe_lba_stats* stats, double* edge_chi2) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "local_bundle_adjustment_mappoints: NULL table");
  if (n_points < 1 || !slot) return fail(ORBFE_ERR_INVALID, "local_bundle_adjustment_mappoints: no slot list");
  const int cap = orbfe_mappoints_capacity(mp);
  for (int p = 0; p < n_points; p++)
    if (slot[p] < 0 || slot[p] >= cap) return fail(ORBFE_ERR_INVALID, "local_bundle_adjustment_mappoints: slot outside [0, capacity)");
  {  // a slot named twice would be written back by two threads
    std::vector<int32_t> sorted(slot, slot + n_points);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end())
      return fail(ORBFE_ERR_INVALID, "local_bundle_adjustment_mappoints: a slot is named twice");
  }
  return run("local_bundle_adjustment_mappoints", 0, mp, slot,
             problem(n_local, n_fixed, Tcw, local_is_fixed, cam, n_points, nullptr, n_edges, edge_pose, edge_point, u, v, u_right, inv_sigma2),
             true, 0, 1, stop_flag, Tcw_out, xw_out, erase, level1, stats, edge_chi2);
}
