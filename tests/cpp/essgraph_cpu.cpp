// Stand-alone program: the arithmetic and work items of csrc/essgraph_math.h -- the very code k_essgraph.hip compiles for the
// device -- under the checks, symbolic factorisation, tables and Levenberg loop of csrc/essgraph_host.h on the CPU, with the
// kernels' summation orders: a block element sums its edges ascending, a factor element takes its updates in ascending
// column order, a wave's sum is 64 lane-strided partial sums combined as the __shfl_down tree does (offsets 32 .. 1).
//   essgraph_cpu opt scene results [repeats]      an optimisation (tests/essgraph_check.py: write_scene / read_result)
//   essgraph_cpu solve system results             orbfe_block_sparse_solve7's operands -> x, ok, blocks_L
// Prints the single-thread time of the best repeat, split by pass.  Build with -ffp-contract=off.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "essgraph_host.h"

using namespace orbfe;

namespace {

template <typename T>
bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n + 1);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
bool wr(std::FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

double tree(double* v) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
  return v[0];
}
double now_us() { return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// k_ess_load + k_ess_factor without the vertices' trials
bool factor_and_solve(const EssArgs& A, double lambda) {
  for (size_t i = 0; i < 49 * (size_t)A.blocksL; i++) ess_load_element(A, i, lambda);
  const int n = A.nFree;
  bool ok = true;
  for (int j = 0; j < n; j++) {
    const int p0 = A.colptr[j], p1 = A.colptr[j + 1];
    for (int i = 0; i < 49 * (p1 - p0); i++) ess_chol_update_element(A.updOff, A.updSrc, A.L, p0 + i / 49, i % 49);
    if (!ess_chol_diag(A.L + 49 * (size_t)p0)) ok = false;
    for (int i = 0; i < 7 * (p1 - p0 - 1); i++) ess_chol_scale_row(A.L + 49 * (size_t)p0, A.L + 49 * (size_t)(p0 + 1 + i / 7), i % 7);
  }
  for (int j = 0; j < n; j++) {
    const int p0 = A.colptr[j], p1 = A.colptr[j + 1];
    ess_fwd_diag(A.L + 49 * (size_t)p0, A.x + 7 * (size_t)j);
    for (int i = 0; i < 7 * (p1 - p0 - 1); i++) {
      const int p = p0 + 1 + i / 7;
      ess_fwd_row(A.L + 49 * (size_t)p, A.x + 7 * (size_t)j, A.x + 7 * (size_t)A.rowidx[p], i % 7);
    }
  }
  for (int j = n - 1; j >= 0; j--) {
    for (int c = 0; c < 7; c++) ess_bwd_component(A.colptr, A.rowidx, A.L, A.x, j, c);
    ess_bwd_diag(A.L + 49 * (size_t)A.colptr[j], A.x + 7 * (size_t)j);
  }
  if (!ok)
    for (int i = 0; i < 7 * n; i++) A.x[i] = 0.0;
  A.rec->ok = ok ? 1 : 0;
  return ok;
}

struct CpuBackend {
  EssArgs A;
  int cur = 0;
  double usLinearise = 0, usSolve = 0, usErrors = 0;

  void record(double lambda, bool setOk) {
    double c[kEssLanes], s[kEssLanes];
    for (int lane = 0; lane < kEssLanes; lane++) ess_record_lane(A, lane, lambda, &c[lane], &s[lane]);
    A.rec->chi2 = tree(c); A.rec->scale = tree(s); A.rec->maxDiag = 0.0; A.rec->nActive = A.nActive;
    if (setOk) A.rec->ok = 1;
  }
  int linearise(LbaRecord* r) {
    const double t0 = now_us();
    for (int k = 0; k < A.nActive; k++) ess_linearise_item(A, k, cur);
    for (int t = 0; t < A.blocksA; t++)
      for (int lane = 0; lane < kEssLanes; lane++) ess_assemble_lane(A, t, lane);
    record(0.0, true);
    usLinearise += now_us() - t0;
    *r = *A.rec;
    return 0;
  }
  int trial(double lambda, LbaRecord* r) {
    const double t0 = now_us();
    factor_and_solve(A, lambda);
    for (int f = 0; f < A.nFree; f++) ess_trial_vertex(A, f, cur);
    const double t1 = now_us();
    for (int k = 0; k < A.nActive; k++) ess_trial_edge(A, k, cur);
    record(lambda, false);
    usSolve += t1 - t0;
    usErrors += now_us() - t1;
    *r = *A.rec;
    return 0;
  }
  void accept() { cur = 1 - cur; }
};

void set_pattern(EssArgs* A, const EssPattern& P) {
  A->colptr = P.colptr.data(); A->rowidx = P.rowidx.data(); A->blockCol = P.blockCol.data();
  A->updOff = P.updOff.data(); A->updSrc = P.updSrc.data(); A->blocksL = P.blocksL();
}

int main_solve(const char* in, const char* out) {
  std::FILE* f = std::fopen(in, "rb");
  if (!f) { std::printf("cannot read %s\n", in); return 2; }
  int32_t hd[2];
  if (std::fread(hd, 4, 2, f) != 2 || hd[0] < 0 || hd[1] < 0) return 2;
  const int n = hd[0], nA = hd[1];
  std::vector<int32_t> colptr, rowidx;
  std::vector<double> blocks, rhs;
  if (!rd(f, colptr, (size_t)n + 1) || !rd(f, rowidx, (size_t)nA) || !rd(f, blocks, 49 * (size_t)nA) || !rd(f, rhs, 7 * (size_t)n)) return 2;
  std::fclose(f);
  if (const char* e = ess_check_pattern(n, colptr.data(), rowidx.data())) { std::printf("refused: %s\n", e); return 1; }
  if (colptr[n] != nA) { std::printf("refused: colptr does not end at the block count\n"); return 1; }
  EssPattern P;
  if (int rc = ess_symbolic(n, colptr.data(), rowidx.data(), &P)) { std::printf("refused: capacity %d\n", rc); return 1; }
  std::vector<double> H(49 * (size_t)P.blocksL(), 0.0), L(H.size()), x(7 * (size_t)n);
  for (int k = 0; k < nA; k++) std::memcpy(H.data() + 49 * (size_t)P.ofA[k], blocks.data() + 49 * (size_t)k, 49 * sizeof(double));
  LbaRecord rec{};
  EssArgs A{};
  A.nFree = n; A.blocksA = nA;
  set_pattern(&A, P);
  A.H = H.data(); A.b = rhs.data(); A.L = L.data(); A.x = x.data(); A.rec = &rec;
  factor_and_solve(A, 0.0);
  std::FILE* g = std::fopen(out, "wb");
  if (!g) return 2;
  const int32_t ints[2] = {rec.ok, P.blocksL()};
  bool ok = wr(g, x.data(), x.size()) && wr(g, ints, 2);
  ok = std::fclose(g) == 0 && ok;
  return ok ? 0 : 2;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 4) { std::printf("usage: essgraph_cpu opt|solve input results [repeats]\n"); return 2; }
  if (std::strcmp(argv[1], "solve") == 0) return main_solve(argv[2], argv[3]);
  const int repeats = argc > 4 ? std::atoi(argv[4]) : 1;
  std::FILE* f = std::fopen(argv[2], "rb");
  if (!f) { std::printf("cannot read %s\n", argv[2]); return 2; }
  int32_t hd[4];
  if (std::fread(hd, 4, 4, f) != 4) return 2;
  const int nV = hd[0], nE = hd[1], fixScale = hd[2], nIt = hd[3];
  if (nV < 0 || nE < 0) return 2;
  std::vector<double> sim3, meas;
  std::vector<uint8_t> fixedFlags, kind;
  std::vector<int32_t> ei, ej;
  if (!rd(f, sim3, 8 * (size_t)nV) || !rd(f, meas, 8 * (size_t)nV) || !rd(f, fixedFlags, (size_t)nV) || !rd(f, ei, (size_t)nE) ||
      !rd(f, ej, (size_t)nE) || !rd(f, kind, (size_t)nE))
    return 2;
  std::fclose(f);
  const EssProblem q{nV, sim3.data(), meas.data(), fixedFlags.data(), nE, ei.data(), ej.data(), kind.data(), fixScale, nIt};
  if (const char* e = ess_check(q)) { std::printf("refused: %s\n", e); return 1; }
  EssTables T;
  if (int rc = ess_build_tables(q, &T)) { std::printf("refused: capacity %d\n", rc); return 1; }
  const size_t nL = (size_t)T.pat.blocksL(), nF = (size_t)T.nFree;
  std::vector<double> est(16 * (size_t)nV + 1), measS(8 * (size_t)nE + 1), lin((size_t)kEssLin * nE + 1), chi2((size_t)nE + 1), H(49 * nL + 1),
      b(7 * nF + 1), L(49 * nL + 1), x(7 * nF + 1);
  LbaRecord rec{};
  EssRun run{};
  CpuBackend be, best;
  double bestUs = 1e300, usTables = 0;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const double t0 = now_us();
    if (rep > 0) ess_build_tables(q, &T);
    usTables = now_us() - t0;
    be = CpuBackend{};
    EssArgs& A = be.A;
    A = EssArgs{};
    A.nVertices = nV; A.nFree = T.nFree; A.nEdges = nE; A.nActive = T.nActive; A.blocksA = T.pat.blocksA(); A.fixScale = fixScale != 0;
    A.sim3 = sim3.data(); A.sim3Meas = meas.data(); A.freeOf = T.freeOf.data(); A.freeVertex = T.freeVertex.data(); A.edgeI = ei.data();
    A.edgeJ = ej.data(); A.edgeKind = kind.data(); A.activeEdge = T.activeEdge.data();
    set_pattern(&A, T.pat);
    A.itemBlock = T.itemBlock.data(); A.itemOff = T.itemOff.data(); A.itemEdge = T.itemEdge.data();
    A.est = est.data(); A.meas = measS.data(); A.lin = lin.data(); A.chi2 = chi2.data(); A.H = H.data(); A.b = b.data(); A.L = L.data();
    A.x = x.data(); A.rec = &rec;
    std::memcpy(est.data(), sim3.data(), 8 * (size_t)nV * sizeof(double));
    std::memcpy(est.data() + 8 * (size_t)nV, sim3.data(), 8 * (size_t)nV * sizeof(double));
    std::fill(H.begin(), H.end(), 0.0); std::fill(b.begin(), b.end(), 0.0); std::fill(x.begin(), x.end(), 0.0);
    for (int e = 0; e < nE; e++) ess_measure_edge(A, e);
    run = EssRun{};
    if (T.nFree > 0 && T.nActive > 0) ess_optimize(be, nIt, &run);
    else run.end = kLbaEndIterations;
    run.syncs++;
    const double us = now_us() - t0;
    if (us < bestUs) { bestUs = us; best = be; }
  }
  const double* he = est.data() + (size_t)be.cur * 8 * (size_t)nV;
  std::vector<float> Tiw(16 * (size_t)nV + 1);
  for (int v = 0; v < nV; v++) ess_Tiw(he + 8 * (size_t)v, Tiw.data() + 16 * (size_t)v);
  std::FILE* g = std::fopen(argv[3], "wb");
  if (!g) return 2;
  const int32_t ints[8] = {run.iterations, run.trials, run.end, run.syncs, T.nFree, T.pat.blocksA(), T.pat.blocksL(), run.solveFailures};
  const double dbl[3] = {run.lambda, run.chi2Initial, run.chi2};
  bool ok = wr(g, he, 8 * (size_t)nV) && wr(g, Tiw.data(), 16 * (size_t)nV) && wr(g, chi2.data(), (size_t)nE) && wr(g, ints, 8) && wr(g, dbl, 3);
  ok = std::fclose(g) == 0 && ok;
  if (!ok) return 2;
  std::printf("vertices=%d edges=%d blocks_A=%d blocks_L=%d cpu_us=%.1f tables_us=%.1f linearise_us=%.1f solve_us=%.1f errors_us=%.1f\n", nV, nE,
              T.pat.blocksA(), T.pat.blocksL(), bestUs, usTables, best.usLinearise, best.usSolve, best.usErrors);
  return 0;
}
