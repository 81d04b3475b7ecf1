// essgraph.hip -- C-ABI entry points of the essential-graph optimisation (include/orbfe.h, "Optimizer::OptimizeEssentialGraph").
// A call is one staged copy up, then g2o's Levenberg loop on the host (essgraph_host.h: ess_optimize) over the kernels of
// k_essgraph.hip on the calling thread's matcher stream: per linearisation and per trial one group of launches and one small
// record back, at the end one copy of the results.  Everything lives in the thread's arena (arena.h: arena_stage): no
// allocation and no event of its own.  The checks, the symbolic factorisation and the tables are essgraph_host.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "essgraph_host.h"
#include "essgraph_kernels.h"
#include "host_internal.h"

using namespace orbfe;

namespace {

struct DeviceBackend {
  Arena* ar = nullptr;
  EssArgs A{};
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
  int linearise(LbaRecord* r) {
    launch_ess_linearise(ar->stream, A, cur);
    return record(r);
  }
  int trial(double lambda, LbaRecord* r) {
    launch_ess_trial(ar->stream, A, cur, lambda);
    return record(r);
  }
  void accept() { cur = 1 - cur; }
};

int capacity_error(const std::string& pre, int rc) {
  if (rc == kEssCapacityBlocks) return fail(ORBFE_ERR_CAPACITY, pre + "the factor has more than 262144 blocks");
  if (rc == kEssCapacityUpdates) return fail(ORBFE_ERR_CAPACITY, pre + "the factorisation has more than 4194304 block updates");
  return fail(ORBFE_ERR_INVALID, pre + "the symbolic factorisation is inconsistent");
}

// the pattern's arrays into the arena
hipError_t stage_pattern(Arena* a, const EssPattern& P, EssArgs* A) {
  int32_t *dcol, *drow, *dbc, *duo, *dus;
  TRY(up(a, &dcol, P.colptr.data(), P.colptr.size()));
  TRY(up(a, &drow, P.rowidx.data(), P.rowidx.size()));
  TRY(up(a, &dbc, P.blockCol.data(), P.blockCol.size()));
  TRY(up(a, &duo, P.updOff.data(), P.updOff.size()));
  TRY(up(a, &dus, P.updSrc.data(), P.updSrc.size()));
  A->colptr = dcol; A->rowidx = drow; A->blockCol = dbc; A->updOff = duo; A->updSrc = dus;
  A->blocksL = P.blocksL();
  return hipSuccess;
}

int check_correction(const std::string& pre, int n_vertices, const double* sim3, const double* sim3_out, int n_points,
                     const int32_t* ref_vertex) {
  if (n_vertices < 1 || n_vertices > kEssMaxVertices) return fail(ORBFE_ERR_INVALID, pre + "n_vertices outside [1, 1048576]");
  if (n_points < 0) return fail(ORBFE_ERR_INVALID, pre + "negative point count");
  if (!sim3 || !sim3_out || (n_points > 0 && !ref_vertex)) return fail(ORBFE_ERR_INVALID, pre + "NULL array");
  if (!ess_all_finite(sim3, 8 * (size_t)n_vertices) || !ess_all_finite(sim3_out, 8 * (size_t)n_vertices))
    return fail(ORBFE_ERR_INVALID, pre + "a sim3 entry is not finite");
  for (int v = 0; v < n_vertices; v++)
    if (!(sim3[8 * (size_t)v + 7] > 0.0) || !(sim3_out[8 * (size_t)v + 7] > 0.0)) return fail(ORBFE_ERR_INVALID, pre + "a scale is not positive");
  for (int p = 0; p < n_points; p++)
    if (ref_vertex[p] < -1 || ref_vertex[p] >= n_vertices) return fail(ORBFE_ERR_INVALID, pre + "ref_vertex outside [-1, n_vertices)");
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_optimize_essential_graph(int device, int n_vertices, const double* sim3, const double* sim3_meas,
                                              const uint8_t* is_fixed, int n_edges, const int32_t* edge_i, const int32_t* edge_j,
                                              const uint8_t* edge_kind, int fix_scale, int n_iterations, double* sim3_out,
                                              float* Tiw_out, double* edge_chi2, orbfe_essgraph_stats* stats) {
  const std::string pre = "optimize_essential_graph: ";
  if (device < 0) return fail(ORBFE_ERR_INVALID, pre + "negative device");
  const EssProblem q{n_vertices, sim3, sim3_meas, is_fixed, n_edges, edge_i, edge_j, edge_kind, fix_scale != 0, n_iterations};
  if (const char* e = ess_check(q)) return fail(ORBFE_ERR_INVALID, pre + e);
  if (!sim3_out || !Tiw_out) return fail(ORBFE_ERR_INVALID, pre + "NULL output array");
  EssTables T;
  if (int rc = ess_build_tables(q, &T)) return capacity_error(pre, rc);
  const size_t nV = (size_t)n_vertices, nE = (size_t)n_edges;
  DeviceBackend be;
  EssArgs& A = be.A;
  A.nVertices = n_vertices; A.nFree = T.nFree; A.nEdges = n_edges; A.nActive = T.nActive; A.blocksA = T.pat.blocksA();
  A.fixScale = fix_scale != 0;
  auto stage = [&](Arena* a) -> hipError_t {
    double *ds, *dm;
    int32_t *dfo, *dfv, *dei, *dej, *dae, *dib, *dio, *die;
    uint8_t* dk;
    TRY(up(a, &ds, sim3, 8 * nV));
    TRY(up(a, &dm, sim3_meas ? sim3_meas : sim3, 8 * nV));
    TRY(up(a, &dfo, T.freeOf.data(), nV));
    TRY(up(a, &dfv, T.freeVertex.data(), T.freeVertex.size()));
    TRY(up(a, &dei, edge_i, nE));
    TRY(up(a, &dej, edge_j, nE));
    if (edge_kind) TRY(up(a, &dk, edge_kind, nE));
    else TRY(up_fill(a, &dk, nE, 0));
    TRY(up(a, &dae, T.activeEdge.data(), T.activeEdge.size()));
    TRY(stage_pattern(a, T.pat, &A));
    TRY(up(a, &dib, T.itemBlock.data(), T.itemBlock.size()));
    TRY(up(a, &dio, T.itemOff.data(), T.itemOff.size()));
    TRY(up(a, &die, T.itemEdge.data(), T.itemEdge.size()));
    TRY(up_fill(a, &A.H, 49 * (size_t)A.blocksL, 0));  // the fill blocks stay 0
    TRY(up_fill(a, &A.b, 7 * (size_t)T.nFree, 0));
    TRY(up_fill(a, &A.x, 7 * (size_t)T.nFree, 0));
    // what travels back: the estimates (both buffers start as the inputs), chi2, the record
    TRY(up_pack(a, &A.est, 16 * nV, [&](double* h) {
      std::memcpy(h, sim3, 8 * nV * sizeof(double));
      std::memcpy(h + 8 * nV, sim3, 8 * nV * sizeof(double));
    }));
    TRY(up_fill(a, &A.chi2, nE, 0));
    TRY(up_fill(a, &A.rec, 1, 0));
    A.sim3 = ds; A.sim3Meas = dm; A.freeOf = dfo; A.freeVertex = dfv; A.edgeI = dei; A.edgeJ = dej; A.edgeKind = dk; A.activeEdge = dae;
    A.itemBlock = dib; A.itemOff = dio; A.itemEdge = die;
    A.meas = carve<double>(a, 8 * nE + 1);
    A.lin = carve<double>(a, (size_t)kEssLin * nE + 1);
    A.L = carve<double>(a, 49 * (size_t)A.blocksL + 1);
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &be.ar, stage));
  HIPCHK(flush(be.ar));
  launch_ess_measure(be.ar->stream, A);
  EssRun run{};
  if (T.nFree > 0 && T.nActive > 0) {
    if (ess_optimize(be, n_iterations, &run)) return fail(hip_status(be.err), pre + hipGetErrorString(be.err));
  } else {
    run.end = kLbaEndIterations;
  }
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(be.ar, A.est, A.rec + 1));
  HIPCHK(hipStreamSynchronize(be.ar->stream));
  run.syncs++;
  const double* he = mirror_of(be.ar, A.est) + (size_t)be.cur * 8 * nV;
  std::memcpy(sim3_out, he, 8 * nV * sizeof(double));
  for (size_t v = 0; v < nV; v++) ess_Tiw(he + 8 * v, Tiw_out + 16 * v);
  if (edge_chi2 && nE) std::memcpy(edge_chi2, mirror_of(be.ar, A.chi2), nE * sizeof(double));
  if (stats) {
    stats->iterations = run.iterations; stats->trials = run.trials; stats->termination = run.end; stats->stopped = 0;
    stats->host_syncs = run.syncs; stats->n_free = T.nFree; stats->blocks_A = T.pat.blocksA(); stats->blocks_L = T.pat.blocksL();
    stats->solve_failures = run.solveFailures; stats->lambda = run.lambda; stats->chi2_initial = run.chi2Initial; stats->chi2 = run.chi2;
  }
  return ORBFE_OK;
}

extern "C" int orbfe_block_sparse_solve7(int device, int n_block_cols, const int32_t* colptr, const int32_t* rowidx, const double* blocks,
                                         const double* rhs, double* x, int32_t* ok, int32_t* blocks_L) {
  const std::string pre = "block_sparse_solve7: ";
  if (device < 0) return fail(ORBFE_ERR_INVALID, pre + "negative device");
  if (const char* e = ess_check_pattern(n_block_cols, colptr, rowidx)) return fail(ORBFE_ERR_INVALID, pre + e);
  if (!blocks || !rhs || !x || !ok) return fail(ORBFE_ERR_INVALID, pre + "NULL array");
  EssPattern P;
  if (int rc = ess_symbolic(n_block_cols, colptr, rowidx, &P)) return capacity_error(pre, rc);
  const size_t nA = (size_t)P.blocksA(), n7 = 7 * (size_t)n_block_cols;
  Arena* ar = nullptr;
  EssArgs A{};
  A.nFree = n_block_cols; A.blocksA = P.blocksA();
  auto stage = [&](Arena* a) -> hipError_t {
    double* db;
    TRY(stage_pattern(a, P, &A));
    TRY(up_pack(a, &A.H, 49 * (size_t)A.blocksL, [&](double* h) {
      std::memset(h, 0, 49 * (size_t)A.blocksL * sizeof(double));
      for (size_t k = 0; k < nA; k++) std::memcpy(h + 49 * (size_t)P.ofA[k], blocks + 49 * k, 49 * sizeof(double));
    }));
    TRY(up(a, &db, rhs, n7));
    A.b = db;
    A.x = carve<double>(a, n7);
    A.rec = carve<LbaRecord>(a, 1);
    A.L = carve<double>(a, 49 * (size_t)A.blocksL + 1);
    // the mirror reaches what travels back (x, rec): the factor behind it never does
    return a->sizing ? hipSuccess : grow_mirror(a, (size_t)(reinterpret_cast<uint8_t*>(A.rec + 1) - a->base.p));
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_ess_solve(ar->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, A.x, A.rec + 1));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(x, mirror_of(ar, A.x), n7 * sizeof(double));
  *ok = mirror_of(ar, A.rec)->ok;
  if (blocks_L) *blocks_L = P.blocksL();
  return ORBFE_OK;
}

extern "C" int orbfe_essential_graph_correct_points(int device, int n_vertices, const double* sim3, const double* sim3_out, int n_points,
                                                    const float* xw, const int32_t* ref_vertex, float* xw_out) {
  const std::string pre = "essential_graph_correct_points: ";
  if (device < 0) return fail(ORBFE_ERR_INVALID, pre + "negative device");
  if (int rc = check_correction(pre, n_vertices, sim3, sim3_out, n_points, ref_vertex)) return rc;
  if (n_points == 0) return ORBFE_OK;
  if (!xw || !xw_out) return fail(ORBFE_ERR_INVALID, pre + "NULL point array");
  const size_t nV = (size_t)n_vertices, nP = (size_t)n_points;
  Arena* ar = nullptr;
  double *ds, *dso;
  float *dx, *dout = nullptr;
  int32_t* dr;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &ds, sim3, 8 * nV));
    TRY(up(a, &dso, sim3_out, 8 * nV));
    TRY(up(a, &dx, xw, 3 * nP));
    TRY(up(a, &dr, ref_vertex, nP));
    dout = carve<float>(a, 3 * nP);
    return a->sizing ? hipSuccess : grow_mirror(a, (size_t)(reinterpret_cast<uint8_t*>(dout + 3 * nP) - a->base.p));
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_ess_correct_points(ar->stream, ds, dso, n_points, dx, dr, dout, nullptr, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, dout, dout + 3 * nP));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(xw_out, mirror_of(ar, dout), 3 * nP * sizeof(float));
  return ORBFE_OK;
}

extern "C" int orbfe_essential_graph_correct_mappoints(orbfe_mappoints* table, int n_vertices, const double* sim3, const double* sim3_out,
                                                       int n_slots, const int32_t* slot, const int32_t* ref_vertex) {
  const std::string pre = "essential_graph_correct_mappoints: ";
  if (!table) return fail(ORBFE_ERR_INVALID, pre + "NULL table");
  if (int rc = check_correction(pre, n_vertices, sim3, sim3_out, n_slots, ref_vertex)) return rc;
  if (n_slots == 0) return ORBFE_OK;
  if (!slot) return fail(ORBFE_ERR_INVALID, pre + "NULL slot list");
  const int cap = orbfe_mappoints_capacity(table);
  for (int p = 0; p < n_slots; p++)
    if (slot[p] < 0 || slot[p] >= cap) return fail(ORBFE_ERR_INVALID, pre + "slot outside [0, capacity)");
  {  // a slot named twice would be rewritten by two lanes
    std::vector<int32_t> sorted(slot, slot + n_slots);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return fail(ORBFE_ERR_INVALID, pre + "a slot is named twice");
  }
  const size_t nV = (size_t)n_vertices, nP = (size_t)n_slots;
  Arena* ar = nullptr;
  double *ds, *dso;
  int32_t *dsl, *dr;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &ds, sim3, 8 * nV));
    TRY(up(a, &dso, sim3_out, 8 * nV));
    TRY(up(a, &dsl, slot, nP));
    TRY(up(a, &dr, ref_vertex, nP));
    return hipSuccess;
  };
  MapPointsLock lock(table);
  if (lock.rc) return lock.rc;
  HIPCHK(arena_stage(lock.device, &ar, stage));
  HIPCHK(flush(ar));
  launch_ess_correct_points(ar->stream, ds, dso, n_slots, nullptr, dr, nullptr, lock.table, dsl);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ar->stream));  // (the lock's scope ends behind the kernel)
  return ORBFE_OK;
}

extern "C" int orbfe_mappoints_positions(orbfe_mappoints* table, int n_slots, const int32_t* slot, float* xw_out) {
  const std::string pre = "mappoints_positions: ";
  if (!table) return fail(ORBFE_ERR_INVALID, pre + "NULL table");
  if (n_slots < 0 || (n_slots > 0 && (!slot || !xw_out))) return fail(ORBFE_ERR_INVALID, pre + "no slot list");
  if (n_slots == 0) return ORBFE_OK;
  const int cap = orbfe_mappoints_capacity(table);
  for (int p = 0; p < n_slots; p++)
    if (slot[p] < 0 || slot[p] >= cap) return fail(ORBFE_ERR_INVALID, pre + "slot outside [0, capacity)");
  const size_t nP = (size_t)n_slots;
  Arena* ar = nullptr;
  int32_t* dsl;
  float* dout = nullptr;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dsl, slot, nP));
    dout = carve<float>(a, 3 * nP);
    return a->sizing ? hipSuccess : grow_mirror(a, (size_t)(reinterpret_cast<uint8_t*>(dout + 3 * nP) - a->base.p));
  };
  MapPointsLock lock(table);
  if (lock.rc) return lock.rc;
  HIPCHK(arena_stage(lock.device, &ar, stage));
  HIPCHK(flush(ar));
  launch_ess_read_positions(ar->stream, *lock.table, dsl, n_slots, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, dout, dout + 3 * nP));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(xw_out, mirror_of(ar, dout), 3 * nP * sizeof(float));
  return ORBFE_OK;
}
