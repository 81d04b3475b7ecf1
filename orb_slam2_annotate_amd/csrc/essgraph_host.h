// essgraph_host.h -- the host side of orbfe_optimize_essential_graph / orbfe_block_sparse_solve7 (essgraph.hip) that needs no
// device: argument checks, the symbolic factorisation of the block graph (elimination tree and column structures of L), the
// tables the kernels read (the edges of a block of H, the update list of a block of L) and g2o's Levenberg loop, written
// over a backend that runs the passes -- the kernels in essgraph.hip, the same work items in a loop in
// tests/cpp/essgraph_cpu.cpp.  Plain C++ without a HIP include, so tests/cpp/essgraph_host_san.cpp runs exactly this code
// under the address and undefined-behaviour sanitizers.
//
// Vertex order: the free vertices keep the caller's order (key-frame ids: a band plus a few dense rows per loop).  There is
// no fill-reducing permutation; blocks_A and blocks_L are reported so that an ordering can be judged.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "essgraph_math.h"

namespace orbfe {

constexpr int kEssMaxVertices = 1 << 20;
constexpr int kEssMaxEdges = 1 << 24;
// Caps with the arena in mind: H and L hold 49 doubles per block of the factor's lower triangle (2 x 98 MB at the cap), the
// update table two int32 per 7 x 7 product of the factorisation (32 MB at the cap).  A 3000-key-frame map with a
// covisibility band of 3 and three loops needs about 3e4 blocks and 1e5 updates.
constexpr int kEssMaxBlocksL = 1 << 18;
constexpr int kEssMaxUpdates = 1 << 22;

enum { kEssOk = 0, kEssCapacityBlocks = 1, kEssCapacityUpdates = 2, kEssInternal = 3 };

struct EssProblem {
  int nVertices;
  const double *sim3, *sim3Meas;  // sim3Meas NULL: the same as sim3
  const uint8_t* isFixed;         // NULL: none
  int nEdges;
  const int32_t *edgeI, *edgeJ;
  const uint8_t* edgeKind;  // NULL: all 0
  int fixScale, nIterations;
};

inline bool ess_all_finite(const double* p, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!(fabs(p[i]) <= DBL_MAX)) return false;
  return true;
}
inline bool ess_is_free(const EssProblem& q, int v) { return !(q.isFixed && q.isFixed[v]); }

// NULL when the operands are fine, else what is wrong with them (one message per check)
inline const char* ess_check(const EssProblem& q) {
  if (q.nVertices < 1) return "n_vertices must be at least 1";
  if (q.nVertices > kEssMaxVertices) return "more than 1048576 vertices";
  if (q.nEdges < 0) return "negative n_edges";
  if (q.nEdges > kEssMaxEdges) return "more than 16777216 edges";
  if (q.nIterations < 0) return "negative n_iterations";
  if (!q.sim3) return "NULL sim3";
  if (q.nEdges > 0 && (!q.edgeI || !q.edgeJ)) return "NULL per-edge array";
  for (int e = 0; e < q.nEdges; e++) {
    if (q.edgeI[e] < 0 || q.edgeI[e] >= q.nVertices || q.edgeJ[e] < 0 || q.edgeJ[e] >= q.nVertices) return "edge index out of range";
    if (q.edgeI[e] == q.edgeJ[e]) return "an edge joins a vertex to itself";
    if (q.edgeKind && q.edgeKind[e] > 1) return "edge_kind must be 0 or 1";
  }
  if (!ess_all_finite(q.sim3, 8 * (size_t)q.nVertices)) return "a sim3 entry is not finite";
  if (q.sim3Meas && !ess_all_finite(q.sim3Meas, 8 * (size_t)q.nVertices)) return "a sim3_meas entry is not finite";
  for (int v = 0; v < q.nVertices; v++) {
    if (!(q.sim3[8 * (size_t)v + 7] > 0.0)) return "a scale of sim3 is not positive";
    if (q.sim3Meas && !(q.sim3Meas[8 * (size_t)v + 7] > 0.0)) return "a scale of sim3_meas is not positive";
  }
  return nullptr;
}

// NULL when (colptr, rowidx) is a block lower-triangular pattern in block-CSC: every column begins with its diagonal block
// and its rows ascend strictly
inline const char* ess_check_pattern(int nCols, const int32_t* colptr, const int32_t* rowidx) {
  if (nCols < 1) return "n_block_cols must be at least 1";
  if (nCols > kEssMaxVertices) return "more than 1048576 block columns";
  if (!colptr || !rowidx) return "NULL pattern";
  if (colptr[0] != 0) return "colptr must begin at 0";
  for (int c = 0; c < nCols; c++) {
    if (colptr[c + 1] <= colptr[c]) return "a column without its diagonal block";
    if (colptr[c + 1] > kEssMaxBlocksL) return "more than 262144 blocks";
    if (rowidx[colptr[c]] != c) return "a column must begin with its diagonal block";
    for (int p = colptr[c] + 1; p < colptr[c + 1]; p++)
      if (rowidx[p] <= rowidx[p - 1] || rowidx[p] >= nCols) return "block rows must ascend strictly below n_block_cols";
  }
  return nullptr;
}

// The pattern of the factor and what the factorisation needs to find its source and target blocks
struct EssPattern {
  int nCols = 0;
  std::vector<int32_t> colptr, rowidx, blockCol;  // L, block-CSC, the diagonal first
  std::vector<int32_t> ofA;                       // [blocks of A]: where block k of the input pattern sits in L
  std::vector<int32_t> updOff, updSrc;            // CSR per block of L: (block (i, k), block (j, k)), k ascending
  int blocksA() const { return (int)ofA.size(); }
  int blocksL() const { return (int)rowidx.size(); }
};

// Symbolic Cholesky on the block graph: struct(L_j) = struct(A_j) joined with struct(L_c) \ {j} of every child c of j in the
// elimination tree (parent(c) = the first off-diagonal row of L_c).  Then the update lists.  kEssOk or what overflowed
inline int ess_symbolic(int nCols, const int32_t* acolptr, const int32_t* arowidx, EssPattern* P) {
  *P = EssPattern{};
  P->nCols = nCols;
  P->colptr.assign((size_t)nCols + 1, 0);
  std::vector<std::vector<int32_t>> pending((size_t)nCols);
  std::vector<int32_t> s;
  for (int j = 0; j < nCols; j++) {
    s.assign(arowidx + acolptr[j] + 1, arowidx + acolptr[j + 1]);
    s.insert(s.end(), pending[j].begin(), pending[j].end());
    std::vector<int32_t>().swap(pending[j]);
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    if (P->rowidx.size() + 1 + s.size() > (size_t)kEssMaxBlocksL) return kEssCapacityBlocks;
    P->rowidx.push_back(j);
    P->rowidx.insert(P->rowidx.end(), s.begin(), s.end());
    P->colptr[(size_t)j + 1] = (int32_t)P->rowidx.size();
    if (!s.empty()) pending[s[0]].insert(pending[s[0]].end(), s.begin() + 1, s.end());
  }
  const int nL = P->blocksL();
  P->blockCol.resize((size_t)nL);
  for (int j = 0; j < nCols; j++)
    for (int p = P->colptr[j]; p < P->colptr[j + 1]; p++) P->blockCol[p] = j;
  // where the blocks of A sit
  P->ofA.resize((size_t)acolptr[nCols]);
  for (int j = 0; j < nCols; j++) {
    int p = P->colptr[j];
    for (int k = acolptr[j]; k < acolptr[j + 1]; k++) {
      while (p < P->colptr[j + 1] && P->rowidx[p] != arowidx[k]) p++;
      if (p == P->colptr[j + 1]) return kEssInternal;
      P->ofA[k] = p;
    }
  }
  // byRow[r]: the off-diagonal blocks of row r, by ascending column
  std::vector<int32_t> rowOff((size_t)nCols + 1, 0), rowBlk;
  for (int p = 0; p < nL; p++)
    if (P->rowidx[p] != P->blockCol[p]) rowOff[(size_t)P->rowidx[p] + 1]++;
  for (int r = 0; r < nCols; r++) rowOff[(size_t)r + 1] += rowOff[r];
  rowBlk.resize((size_t)rowOff[nCols]);
  {
    std::vector<int32_t> cur(rowOff.begin(), rowOff.end() - 1);
    for (int p = 0; p < nL; p++)
      if (P->rowidx[p] != P->blockCol[p]) rowBlk[cur[P->rowidx[p]]++] = p;
  }
  std::vector<int32_t> pos((size_t)nCols, -1);
  P->updOff.assign((size_t)nL + 1, 0);
  for (int pass = 0; pass < 2; pass++) {
    std::vector<int32_t> cur;
    if (pass == 1) {
      size_t total = 0;
      for (int p = 0; p < nL; p++) {
        const size_t n = (size_t)P->updOff[(size_t)p + 1];
        P->updOff[p] = (int32_t)total;
        total += n;
        if (total > (size_t)kEssMaxUpdates) return kEssCapacityUpdates;
      }
      P->updOff[nL] = (int32_t)total;
      P->updSrc.assign(2 * total, 0);
      cur.assign(P->updOff.begin(), P->updOff.end() - 1);
    }
    for (int j = 0; j < nCols; j++) {
      for (int p = P->colptr[j]; p < P->colptr[j + 1]; p++) pos[P->rowidx[p]] = p;
      for (int t = rowOff[j]; t < rowOff[(size_t)j + 1]; t++) {
        const int pjk = rowBlk[t], k = P->blockCol[pjk];
        for (int pik = pjk; pik < P->colptr[k + 1]; pik++) {  // rows ascend: from (j, k) down the column
          const int target = pos[P->rowidx[pik]];
          if (target < 0) return kEssInternal;
          if (pass == 0) {
            P->updOff[(size_t)target + 1]++;
          } else {
            P->updSrc[2 * (size_t)cur[target]] = pik;
            P->updSrc[2 * (size_t)cur[target] + 1] = pjk;
            cur[target]++;
          }
        }
      }
      for (int p = P->colptr[j]; p < P->colptr[j + 1]; p++) pos[P->rowidx[p]] = -1;
    }
    if (pass == 0) {  // counts sit at [p + 1]; the second pass turns them into offsets
      size_t total = 0;
      for (int p = 0; p < nL; p++) total += (size_t)P->updOff[(size_t)p + 1];
      if (total > (size_t)kEssMaxUpdates) return kEssCapacityUpdates;
    }
  }
  return kEssOk;
}

// The tables of an optimisation: functions of the problem's shape only
struct EssTables {
  int nFree = 0, nActive = 0;
  std::vector<int32_t> freeOf, freeVertex, activeEdge;
  EssPattern pat;
  std::vector<int32_t> itemBlock, itemOff, itemEdge;
};

inline int ess_build_tables(const EssProblem& q, EssTables* T) {
  *T = EssTables{};
  T->freeOf.resize((size_t)q.nVertices);
  for (int v = 0; v < q.nVertices; v++) {
    T->freeOf[v] = ess_is_free(q, v) ? T->nFree++ : -1;
    if (T->freeOf[v] >= 0) T->freeVertex.push_back(v);
  }
  const int nF = T->nFree;
  // an edge between two fixed vertices is not active (sparse_optimizer.cpp:234)
  std::vector<int32_t> deg((size_t)nF + 1, 0);
  struct Pair { int32_t col, row, edge; };
  std::vector<Pair> pairs;
  for (int e = 0; e < q.nEdges; e++) {
    const int fi = T->freeOf[q.edgeI[e]], fj = T->freeOf[q.edgeJ[e]];
    if (fi < 0 && fj < 0) continue;
    T->activeEdge.push_back(e);
    if (fi >= 0) deg[(size_t)fi + 1]++;
    if (fj >= 0) deg[(size_t)fj + 1]++;
    if (fi >= 0 && fj >= 0) pairs.push_back(Pair{std::min(fi, fj), std::max(fi, fj), e});
  }
  T->nActive = (int)T->activeEdge.size();
  if (nF == 0) return kEssOk;
  std::sort(pairs.begin(), pairs.end(), [](const Pair& a, const Pair& b) {
    return a.col != b.col ? a.col < b.col : a.row != b.row ? a.row < b.row : a.edge < b.edge;
  });
  // the pattern of H: per column the diagonal, then the rows of its pairs
  std::vector<int32_t> acol((size_t)nF + 1, 0), arow;
  {
    size_t k = 0;
    for (int c = 0; c < nF; c++) {
      arow.push_back(c);
      for (; k < pairs.size() && pairs[k].col == c; k++)
        if (arow.back() != pairs[k].row) arow.push_back(pairs[k].row);
      if (arow.size() > (size_t)kEssMaxBlocksL) return kEssCapacityBlocks;
      acol[(size_t)c + 1] = (int32_t)arow.size();
    }
  }
  if (int rc = ess_symbolic(nF, acol.data(), arow.data(), &T->pat)) return rc;
  // the edges of the diagonal blocks: CSR by free vertex, ascending edge id
  for (int f = 0; f < nF; f++) deg[(size_t)f + 1] += deg[f];
  std::vector<int32_t> vertEdge((size_t)deg[nF]), cur(deg.begin(), deg.end() - 1);
  for (int e : T->activeEdge) {
    const int fi = T->freeOf[q.edgeI[e]], fj = T->freeOf[q.edgeJ[e]];
    if (fi >= 0) vertEdge[cur[fi]++] = e;
    if (fj >= 0) vertEdge[cur[fj]++] = e;
  }
  T->itemBlock = T->pat.ofA;
  T->itemOff.push_back(0);
  size_t k = 0;
  for (int c = 0; c < nF; c++) {
    for (int a = acol[c]; a < acol[(size_t)c + 1]; a++) {
      if (arow[a] == c) {
        T->itemEdge.insert(T->itemEdge.end(), vertEdge.begin() + deg[c], vertEdge.begin() + deg[(size_t)c + 1]);
      } else {
        for (; k < pairs.size() && pairs[k].col == c && pairs[k].row == arow[a]; k++) T->itemEdge.push_back(pairs[k].edge);
      }
      T->itemOff.push_back((int32_t)T->itemEdge.size());
    }
  }
  return kEssOk;
}

// ---- the schedule ----
struct EssRun {
  int32_t iterations = 0, trials = 0, end = 0, syncs = 0, solveFailures = 0;
  double lambda = 0.0, chi2Initial = 0.0, chi2 = 0.0;
};

// optimize(maxIt) of SparseOptimizer with OptimizationAlgorithmLevenberg and the user's lambda_init.  B: linearise(&rec),
// trial(lambda, &rec), accept() -- 0 or an error code.  One record back per group of launches
template <typename B>
int ess_optimize(B& be, int maxIt, EssRun* run) {
  *run = EssRun{};
  LbaLM lm;
  lba_lm_begin(&lm, maxIt);
  LbaRecord rec;
  bool more = maxIt > 0;
  if (!more) lm.end = kLbaEndIterations;
  while (more) {
    if (int rc = be.linearise(&rec)) return rc;
    run->syncs++;
    if (lm.it == 0) run->chi2Initial = rec.chi2;
    ess_lm_after_linearise(&lm, rec);
    do {
      if (int rc = be.trial(lm.lam, &rec)) return rc;
      run->syncs++;
      if (!rec.ok) run->solveFailures++;  // a zero step and a rejected trial
      if (lba_lm_after_trial(&lm, rec)) be.accept();
    } while (lba_lm_more_trials(lm));
    more = lba_lm_after_iteration(&lm);
  }
  run->iterations = lm.it; run->trials = lm.trials; run->end = lm.end; run->lambda = lm.lam; run->chi2 = lm.cur;
  return 0;
}

}  // namespace orbfe
