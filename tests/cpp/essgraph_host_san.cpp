// Stand-alone program: the host side of orbfe_optimize_essential_graph / orbfe_block_sparse_solve7 (csrc/essgraph_host.h: the
// argument checks, the symbolic factorisation, the table builders) on exactly-sized heap buffers, and the factorisation's
// element operations driven through those tables, up to where the entry points would make their first device call.  Built
// with -fsanitize=address,undefined and run on the CPU (tests/test_essgraph_host_san.py); nothing of it is loaded into
// Python.  Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>
#include <set>
#include <utility>
#include <vector>

#include "essgraph_host.h"

using namespace orbfe;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)
#define SAYS(expr, text)                                                 \
  do {                                                                   \
    const char* _m = (expr);                                             \
    if (!_m || std::strcmp(_m, text) != 0) { std::printf("FAILED %s:%d: %s gave %s\n", __FILE__, __LINE__, #expr, _m ? _m : "NULL"); return 1; } \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

// a graph on exactly-sized arrays: identity rotations, vertex v at x = v, scale 1
struct Graph {
  int n, nE;
  std::unique_ptr<double[]> sim3, meas;
  std::unique_ptr<uint8_t[]> fixedFlags, kind;
  std::unique_ptr<int32_t[]> ei, ej;
  Graph(int n_, const std::vector<std::pair<int, int>>& edges, const std::vector<int>& fixed) : n(n_), nE((int)edges.size()) {
    sim3 = exact<double>(8 * (size_t)n); meas = exact<double>(8 * (size_t)n);
    fixedFlags = exact<uint8_t>(n); kind = exact<uint8_t>(nE); ei = exact<int32_t>(nE); ej = exact<int32_t>(nE);
    for (int v = 0; v < n; v++) {
      sim3[8 * (size_t)v + 3] = 1.0; sim3[8 * (size_t)v + 4] = (double)v; sim3[8 * (size_t)v + 7] = 1.0;
      meas[8 * (size_t)v + 3] = 1.0; meas[8 * (size_t)v + 4] = 1.01 * (double)v; meas[8 * (size_t)v + 7] = 1.0;
    }
    for (int f : fixed) fixedFlags[f] = 1;
    for (int e = 0; e < nE; e++) { ei[e] = edges[e].first; ej[e] = edges[e].second; kind[e] = (uint8_t)(e % 2); }
  }
  EssProblem q(int nIt = 5) const { return EssProblem{n, sim3.get(), meas.get(), fixedFlags.get(), nE, ei.get(), ej.get(), kind.get(), 0, nIt}; }
};

static std::vector<std::pair<int, int>> chain(int n, int band) {
  std::vector<std::pair<int, int>> e;
  for (int k = 0; k < n; k++)
    for (int d = 1; d <= band; d++)
      if (k + d < n) e.push_back({k, k + d});
  return e;
}

// the tables of q against the definitions they are built from
static int check_tables(const Graph& G) {
  const EssProblem q = G.q();
  EXPECT(ess_check(q) == nullptr);
  EssTables T;
  EXPECT(ess_build_tables(q, &T) == kEssOk);
  const EssPattern& P = T.pat;
  const int nF = T.nFree;
  int nFreeWant = 0;
  for (int v = 0; v < G.n; v++) {
    if (!G.fixedFlags[v]) { EXPECT(T.freeOf[v] == nFreeWant); EXPECT(T.freeVertex[nFreeWant] == v); nFreeWant++; }
    else EXPECT(T.freeOf[v] == -1);
  }
  EXPECT(nF == nFreeWant);
  if (nF == 0) { EXPECT(T.nActive == 0 && P.blocksL() == 0); return 0; }
  // the pattern of H from the definition, and the elimination game on it
  std::vector<std::set<int>> cols((size_t)nF);
  std::set<std::pair<int, int>> blocksA;
  int nActive = 0;
  for (int e = 0; e < G.nE; e++) {
    const int fi = T.freeOf[G.ei[e]], fj = T.freeOf[G.ej[e]];
    if (fi < 0 && fj < 0) continue;
    EXPECT(T.activeEdge[nActive] == e);
    nActive++;
    if (fi >= 0 && fj >= 0) { cols[std::min(fi, fj)].insert(std::max(fi, fj)); blocksA.insert({std::min(fi, fj), std::max(fi, fj)}); }
  }
  EXPECT(nActive == T.nActive);
  EXPECT(P.blocksA() == nF + (int)blocksA.size());
  EXPECT((int)P.colptr.size() == nF + 1 && P.colptr[0] == 0 && P.colptr[nF] == P.blocksL());
  for (int j = 0; j < nF; j++) {
    EXPECT(P.rowidx[P.colptr[j]] == j);
    std::vector<int> rows(cols[j].begin(), cols[j].end());
    EXPECT(P.colptr[j + 1] - P.colptr[j] == 1 + (int)rows.size());
    for (size_t k = 0; k < rows.size(); k++) {
      EXPECT(P.rowidx[P.colptr[j] + 1 + (int)k] == rows[k]);
      for (size_t m = k + 1; m < rows.size(); m++) cols[rows[k]].insert(rows[m]);
    }
    for (int p = P.colptr[j]; p < P.colptr[j + 1]; p++) EXPECT(P.blockCol[p] == j);
  }
  // every update names blocks (i, k), (j, k) of one earlier column, k ascending, and every such pair is listed
  size_t nUpd = 0;
  for (int k = 0; k < nF; k++) {
    const size_t m = (size_t)(P.colptr[k + 1] - P.colptr[k] - 1);
    nUpd += m * (m + 1) / 2;
  }
  EXPECT((size_t)P.updOff[P.blocksL()] == nUpd && P.updSrc.size() == 2 * nUpd);
  for (int p = 0; p < P.blocksL(); p++) {
    int last = -1;
    for (int u = P.updOff[p]; u < P.updOff[p + 1]; u++) {
      const int a = P.updSrc[2 * (size_t)u], b = P.updSrc[2 * (size_t)u + 1];
      EXPECT(a >= 0 && a < P.blocksL() && b >= 0 && b < P.blocksL());
      EXPECT(P.blockCol[a] == P.blockCol[b] && P.blockCol[a] < P.blockCol[p] && P.blockCol[a] > last);
      EXPECT(P.rowidx[a] == P.rowidx[p] && P.rowidx[b] == P.blockCol[p]);
      last = P.blockCol[a];
    }
  }
  // the items: the blocks of H with their edges, ascending
  EXPECT((int)T.itemBlock.size() == P.blocksA() && (int)T.itemOff.size() == P.blocksA() + 1);
  size_t seen = 0;
  for (int t = 0; t < P.blocksA(); t++) {
    const int p = T.itemBlock[t];
    EXPECT(p >= 0 && p < P.blocksL());
    const int vr = T.freeVertex[P.rowidx[p]], vc = T.freeVertex[P.blockCol[p]];
    int last = -1;
    for (int k = T.itemOff[t]; k < T.itemOff[t + 1]; k++) {
      const int e = T.itemEdge[k];
      EXPECT(e > last && e < G.nE);
      last = e;
      if (vr == vc) EXPECT(G.ei[e] == vr || G.ej[e] == vr);
      else EXPECT((G.ei[e] == vr && G.ej[e] == vc) || (G.ei[e] == vc && G.ej[e] == vr));
      seen++;
    }
    if (vr != vc) EXPECT(T.itemOff[t + 1] > T.itemOff[t]);
  }
  size_t want = 0;
  for (int e = 0; e < G.nE; e++) {
    const int fi = T.freeOf[G.ei[e]], fj = T.freeOf[G.ej[e]];
    want += (fi >= 0) + (fj >= 0) + (fi >= 0 && fj >= 0);
  }
  EXPECT(seen == want && T.itemEdge.size() == want);
  // the element operations through the tables, on exactly-sized H / L / x: a diagonally dominant matrix on the pattern
  const size_t nL = (size_t)P.blocksL();
  auto H = exact<double>(49 * nL), L = exact<double>(49 * nL), b = exact<double>(7 * (size_t)nF), x = exact<double>(7 * (size_t)nF);
  for (int t = 0; t < P.blocksA(); t++) {
    const int p = T.itemBlock[t];
    for (int el = 0; el < 49; el++) {
      const int r = el / 7, c = el % 7;
      if (P.rowidx[p] == P.blockCol[p]) H[49 * (size_t)p + el] = r == c ? 40.0 + p % 5 : 0.25 / (1 + (r > c ? r - c : c - r));
      else H[49 * (size_t)p + el] = 0.125 * ((r + 2 * c + p) % 5 - 2);
    }
  }
  for (int i = 0; i < 7 * nF; i++) b[i] = 1.0 + 0.01 * (i % 13);
  LbaRecord rec{};
  EssArgs A{};
  A.nFree = nF; A.blocksA = P.blocksA(); A.blocksL = P.blocksL();
  A.colptr = P.colptr.data(); A.rowidx = P.rowidx.data(); A.blockCol = P.blockCol.data(); A.updOff = P.updOff.data(); A.updSrc = P.updSrc.data();
  A.H = H.get(); A.b = b.get(); A.L = L.get(); A.x = x.get(); A.rec = &rec;
  for (size_t i = 0; i < 49 * nL; i++) ess_load_element(A, i, 0.5);
  bool ok = true;
  for (int j = 0; j < nF; j++) {
    const int p0 = P.colptr[j], p1 = P.colptr[j + 1];
    for (int i = 0; i < 49 * (p1 - p0); i++) ess_chol_update_element(A.updOff, A.updSrc, A.L, p0 + i / 49, i % 49);
    ok = ess_chol_diag(A.L + 49 * (size_t)p0) && ok;
    for (int i = 0; i < 7 * (p1 - p0 - 1); i++) ess_chol_scale_row(A.L + 49 * (size_t)p0, A.L + 49 * (size_t)(p0 + 1 + i / 7), i % 7);
  }
  EXPECT(ok);
  for (int j = 0; j < nF; j++) {
    const int p0 = P.colptr[j], p1 = P.colptr[j + 1];
    ess_fwd_diag(A.L + 49 * (size_t)p0, A.x + 7 * (size_t)j);
    for (int i = 0; i < 7 * (p1 - p0 - 1); i++)
      ess_fwd_row(A.L + 49 * (size_t)(p0 + 1 + i / 7), A.x + 7 * (size_t)j, A.x + 7 * (size_t)P.rowidx[p0 + 1 + i / 7], i % 7);
  }
  for (int j = nF - 1; j >= 0; j--) {
    for (int c = 0; c < 7; c++) ess_bwd_component(A.colptr, A.rowidx, A.L, A.x, j, c);
    ess_bwd_diag(A.L + 49 * (size_t)P.colptr[j], A.x + 7 * (size_t)j);
  }
  // the residual of (H + 0.5 I) x = b, H symmetric from its lower blocks (a diagonal block from its lower triangle)
  std::vector<double> r(b.get(), b.get() + 7 * (size_t)nF);
  for (int p = 0; p < P.blocksL(); p++) {
    const int row = P.rowidx[p], col = P.blockCol[p];
    for (int a = 0; a < 7; a++)
      for (int c = 0; c < 7; c++) {
        if (row == col) {
          const double h = (a >= c ? H[49 * (size_t)p + 7 * a + c] : H[49 * (size_t)p + 7 * c + a]) + (a == c ? 0.5 : 0.0);
          r[7 * (size_t)row + a] -= h * x[7 * (size_t)col + c];
        } else {
          const double h = H[49 * (size_t)p + 7 * a + c];
          r[7 * (size_t)row + a] -= h * x[7 * (size_t)col + c];
          r[7 * (size_t)col + c] -= h * x[7 * (size_t)row + a];
        }
      }
  }
  for (double v : r) EXPECT(std::fabs(v) < 1e-9);
  return 0;
}

int main() {
  // the scenes' shapes: chains, a fixed vertex in the middle with an isolated vertex, rings with loop bundles and duplicates,
  // a band of 3 over more block columns than a wave has lanes, sizes on and around a wave
  {
    Graph G(5, chain(5, 1), {0});
    if (check_tables(G)) return 1;
  }
  {
    Graph G(6, chain(5, 1), {2});
    if (check_tables(G)) return 1;
  }
  {
    auto e = chain(12, 1);
    for (auto p : {std::pair<int, int>{10, 0}, {10, 1}, {11, 0}, {11, 1}, {3, 4}, {10, 1}, {2, 7}}) e.push_back(p);
    Graph G(12, e, {0});
    if (check_tables(G)) return 1;
    Graph G2(12, e, {5, 11});
    if (check_tables(G2)) return 1;
  }
  for (int n : {63, 64, 65, 150}) {
    auto e = chain(n, 3);
    for (auto p : {std::pair<int, int>{n - 2, 0}, {n - 2, 1}, {n - 1, 0}, {n - 1, 1}, {n - 5, 30}, {n - 4, 31}}) e.push_back(p);
    Graph G(n, e, {0});
    if (check_tables(G)) return 1;
  }
  {  // no free vertex; no edge at all
    Graph G(3, chain(3, 1), {0, 1, 2});
    if (check_tables(G)) return 1;
    Graph G2(4, {}, {});
    if (check_tables(G2)) return 1;
  }
  // every refused input, each with its own message
  {
    Graph G(5, chain(5, 1), {0});
    EssProblem q = G.q();
    q.nVertices = 0;
    SAYS(ess_check(q), "n_vertices must be at least 1");
    q = G.q(-1);
    SAYS(ess_check(q), "negative n_iterations");
    q = G.q(); q.nEdges = -1;
    SAYS(ess_check(q), "negative n_edges");
    q = G.q(); q.sim3 = nullptr;
    SAYS(ess_check(q), "NULL sim3");
    q = G.q(); q.edgeJ = nullptr;
    SAYS(ess_check(q), "NULL per-edge array");
    G.ej[2] = G.ei[2];
    SAYS(ess_check(G.q()), "an edge joins a vertex to itself");
    G.ej[2] = 5;
    SAYS(ess_check(G.q()), "edge index out of range");
    G.ej[2] = -1;
    SAYS(ess_check(G.q()), "edge index out of range");
    G.ej[2] = 3;
    G.kind[1] = 2;
    SAYS(ess_check(G.q()), "edge_kind must be 0 or 1");
    G.kind[1] = 1;
    G.sim3[8 * 4 + 5] = std::numeric_limits<double>::quiet_NaN();
    SAYS(ess_check(G.q()), "a sim3 entry is not finite");
    G.sim3[8 * 4 + 5] = 0.0;
    G.meas[8 * 4 + 7] = std::numeric_limits<double>::infinity();
    SAYS(ess_check(G.q()), "a sim3_meas entry is not finite");
    G.meas[8 * 4 + 7] = 1.0;
    G.sim3[8 * 4 + 7] = 0.0;
    SAYS(ess_check(G.q()), "a scale of sim3 is not positive");
    G.sim3[8 * 4 + 7] = 1.0;
    G.meas[8 * 2 + 7] = -1.0;
    SAYS(ess_check(G.q()), "a scale of sim3_meas is not positive");
    G.meas[8 * 2 + 7] = 1.0;
    EXPECT(ess_check(G.q()) == nullptr);
    q = G.q(); q.sim3Meas = nullptr; q.isFixed = nullptr; q.edgeKind = nullptr;
    EXPECT(ess_check(q) == nullptr);
    EssTables T;
    EXPECT(ess_build_tables(q, &T) == kEssOk && T.nFree == 5);
  }
  {  // the pattern of orbfe_block_sparse_solve7
    const int32_t colptr[4] = {0, 2, 4, 5}, rowidx[5] = {0, 2, 1, 2, 2};
    EXPECT(ess_check_pattern(3, colptr, rowidx) == nullptr);
    EssPattern P;
    EXPECT(ess_symbolic(3, colptr, rowidx, &P) == kEssOk && P.blocksL() == 5 && P.blocksA() == 5);
    SAYS(ess_check_pattern(0, colptr, rowidx), "n_block_cols must be at least 1");
    SAYS(ess_check_pattern(3, nullptr, rowidx), "NULL pattern");
    const int32_t c1[4] = {1, 2, 4, 5};
    SAYS(ess_check_pattern(3, c1, rowidx), "colptr must begin at 0");
    const int32_t c2[4] = {0, 2, 2, 5};
    SAYS(ess_check_pattern(3, c2, rowidx), "a column without its diagonal block");
    const int32_t r1[5] = {0, 2, 2, 2, 2};
    SAYS(ess_check_pattern(3, colptr, r1), "a column must begin with its diagonal block");
    const int32_t r2[5] = {0, 3, 1, 2, 2};
    SAYS(ess_check_pattern(3, colptr, r2), "block rows must ascend strictly below n_block_cols");
    const int32_t c3[3] = {0, 3, 4}, r3[4] = {0, 1, 1, 1};
    SAYS(ess_check_pattern(2, c3, r3), "block rows must ascend strictly below n_block_cols");
  }
  std::printf("ok\n");
  return 0;
}
