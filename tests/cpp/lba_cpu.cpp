// Stand-alone program: the arithmetic and work items of csrc/lba_math.h -- the very code k_lba.hip compiles for the device --
// under the schedule, checks and index arrays of csrc/lba_host.h on the CPU, with the kernels' summation orders: a wave's sum
// is 64 lane-strided partial sums combined as the __shfl_down tree does (offsets 32 .. 1, lane 0's total); the dense solve
// runs its element operations in elimination order.  Reads a scene file (tests/test_lba_math_cpu.py: write_scene), writes the
// results, and prints the single-thread time of the best repeat.  Build with -ffp-contract=off.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lba_host.h"

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
double tree_max(double* v) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int l = 0; l < off; l++) v[l] = fmax(v[l], v[l + off]);
  return v[0];
}

struct CpuBackend {
  LbaArgs A;
  std::vector<uint8_t>* erase;
  int cur = 0, linearised = 0;

  void record(bool setOk) {
    double c[kLbaLanes], s[kLbaLanes], m[kLbaLanes];
    int n = 0;
    for (int lane = 0; lane < kLbaLanes; lane++) {
      LbaTotals t;
      lba_totals_lane(A, lane, &t);
      c[lane] = t.chi2; s[lane] = t.scale; m[lane] = t.maxDiag; n += t.nActive;
    }
    A.rec->chi2 = tree(c); A.rec->scale = tree(s); A.rec->maxDiag = tree_max(m); A.rec->nActive = n;
    if (setOk) A.rec->ok = 1;
  }
  int linearise(bool robust, LbaRecord* r) {
    linearised++;
    for (int p = 0; p < A.nPoints; p++) lba_linearise_point(A, p, cur, robust);
    for (int f = 0; f < A.nFree; f++) {
      static double part[kLbaPoseSums][kLbaLanes];
      int n = 0;
      for (int lane = 0; lane < kLbaLanes; lane++) {
        double acc[kLbaPoseSums];
        int k;
        lba_pose_block_lane(A, f, lane, acc, &k);
        n += k;
        for (int i = 0; i < kLbaPoseSums; i++) part[i][lane] = acc[i];
      }
      double tot[kLbaPoseSums];
      for (int i = 0; i < kLbaPoseSums; i++) tot[i] = tree(part[i]);
      lba_pose_block_finish(A, f, tot, n);
    }
    record(true);
    *r = *A.rec;
    return 0;
  }
  int trial(double lambda, bool robust, LbaRecord* r) {
    for (int p = 0; p < A.nPoints; p++) lba_schur_point(A, p, lambda);
    const int nBlocks = lba_count_blocks(A.nFree);
    for (int b = 0; b < nBlocks; b++) {
      static double part[kLbaBlockSums][kLbaLanes];
      const int i1 = A.blockPose[2 * b], i2 = A.blockPose[2 * b + 1];
      for (int lane = 0; lane < kLbaLanes; lane++) {
        double acc[kLbaBlockSums];
        lba_schur_block_lane(A, i1, i2, lane, acc);
        for (int i = 0; i < kLbaBlockSums; i++) part[i][lane] = acc[i];
      }
      double tot[kLbaBlockSums];
      for (int i = 0; i < kLbaBlockSums; i++) tot[i] = tree(part[i]);
      lba_schur_block_finish(A, i1, i2, tot, lambda);
    }
    for (int f = 0; f < A.nFree; f++) {
      static double part[6][kLbaLanes];
      for (int lane = 0; lane < kLbaLanes; lane++) {
        double acc[6];
        lba_schur_rhs_lane(A, f, lane, acc);
        for (int i = 0; i < 6; i++) part[i][lane] = acc[i];
      }
      double tot[6];
      for (int i = 0; i < 6; i++) tot[i] = tree(part[i]);
      lba_schur_rhs_finish(A, f, tot);
    }
    // k_lba_solve
    const size_t n = 6 * (size_t)A.nFree;
    double* S = A.S;
    bool ok = true;
    for (size_t j = 0; j < n && ok; j++) {
      if (!lba_chol_pivot(S, n, j)) { ok = false; break; }
      for (size_t i = j + 1; i < n; i++) lba_chol_scale(S, n, j, i);
      for (size_t i = j + 1; i < n; i++)
        for (size_t k = j + 1; k <= i; k++) lba_chol_update(S, n, j, i, k);
    }
    if (ok) {
      double* y = A.bs;
      for (size_t j = 0; j < n; j++) {
        y[j] = y[j] / S[j * n + j];
        for (size_t i = j + 1; i < n; i++) y[i] = y[i] - S[i * n + j] * y[j];
      }
      for (size_t jj = n; jj > 0; jj--) {
        const size_t j = jj - 1;
        y[j] = y[j] / S[j * n + j];
        for (size_t i = 0; i < j; i++) y[i] = y[i] - S[j * n + i] * y[j];
      }
      for (size_t i = 0; i < n; i++) A.xp[i] = y[i];
    } else {
      for (size_t i = 0; i < n; i++) A.xp[i] = 0.0;
    }
    A.rec->ok = ok ? 1 : 0;
    for (int j = 0; j < A.nPoses; j++) lba_pose_trial(A, j, cur, lambda);
    for (int p = 0; p < A.nPoints; p++) lba_trial_point(A, p, cur, lambda, robust, ok);
    record(false);
    *r = *A.rec;
    return 0;
  }
  void accept() { cur = 1 - cur; }
  int classify(bool final) {
    for (int e = 0; e < A.nEdges; e++) {
      const bool bad = lba_edge_bad(A, e, cur);
      if (final) (*erase)[e] = bad ? (A.level[e] != 0 ? 1 : 2) : 0;
      else if (bad) A.level[e] = 1;
    }
    return 0;
  }
};

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: lba_cpu scene results [repeats]\n"); return 2; }
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 1;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  int32_t hd[9];
  if (std::fread(hd, 4, 9, f) != 9) return 2;
  const int nLocal = hd[0], nFixed = hd[1], nPoints = hd[2], nEdges = hd[3], hasFixed = hd[4], global = hd[5], nIt = hd[6], robust = hd[7],
            stopBefore = hd[8];
  if (nLocal < 0 || nFixed < 0 || nPoints < 0 || nEdges < 0) return 2;
  const size_t nT = (size_t)nLocal + nFixed, nP = (size_t)nPoints, nE = (size_t)nEdges;
  std::vector<float> Tcw, cam, xw, u, v, ur, w;
  std::vector<uint8_t> fixedFlags;
  std::vector<int32_t> ep, ept;
  if (!rd(f, Tcw, 16 * nT) || !rd(f, fixedFlags, (size_t)nLocal) || !rd(f, cam, 5 * nT) || !rd(f, xw, 3 * nP) || !rd(f, ep, nE) ||
      !rd(f, ept, nE) || !rd(f, u, nE) || !rd(f, v, nE) || !rd(f, ur, nE) || !rd(f, w, nE))
    return 2;
  std::fclose(f);
  const LbaProblem q{nLocal, nFixed, Tcw.data(), hasFixed ? fixedFlags.data() : nullptr, cam.data(), nPoints, xw.data(), nEdges,
                     ep.data(), ept.data(), u.data(), v.data(), ur.data(), w.data()};
  if (const char* e = lba_check(q, false)) { std::printf("refused: %s\n", e); return 1; }
  const int nFree = lba_count_free(q), nBlocks = lba_count_blocks(nFree);
  const size_t n6 = 6 * (size_t)nFree;
  std::vector<float> cam8(8 * nT), obs(4 * nE);
  std::vector<int32_t> freeOf(nT), ptOff(nP + 1), poseOff((size_t)nFree + 1), poseEdge((size_t)lba_count_free_edges(q) + 1),
      edgeOf((size_t)nFree * nP + 1), blockPose(2 * (size_t)nBlocks + 1);
  std::vector<double> pose(16 * nT), pt(6 * nP), chi2(nE), lin(kLbaLin * nE), Y(18 * nE), Hll(6 * nP), bl(3 * nP), HllInv(6 * nP),
      Db(3 * nP), ptRho(nP), ptScale(nP), Hpp(21 * (size_t)nFree + 1), bp(n6 + 1), poseScale((size_t)nFree + 1), S(n6 * n6 + 1), bs(n6 + 1),
      xp(n6 + 1);
  std::vector<uint8_t> level(nE), ptAct(nP), poseAct((size_t)nFree + 1), erase(nE);
  LbaRecord rec{};
  LbaRun run{};
  CpuBackend be;
  bool seen = false;
  double bestUs = 1e300;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    lba_pack_cam(cam8.data(), q); lba_pack_obs(obs.data(), q); lba_fill_free_of(freeOf.data(), q); lba_fill_pt_off(ptOff.data(), q);
    lba_fill_pose_off(poseOff.data(), q); lba_fill_pose_edge(poseEdge.data(), q); lba_fill_edge_of(edgeOf.data(), q);
    lba_fill_blocks(blockPose.data(), nFree);
    lba_pack_poses(pose.data(), q); lba_pack_poses(pose.data() + 8 * nT, q);
    lba_pack_points(pt.data(), q); lba_pack_points(pt.data() + 3 * nP, q);
    for (size_t e = 0; e < nE; e++) { level[e] = 0; chi2[e] = 0.0; erase[e] = 0; }
    be = CpuBackend{};
    LbaArgs& A = be.A;
    A = LbaArgs{};
    A.nPoses = (int)nT; A.nFree = nFree; A.nPoints = nPoints; A.nEdges = nEdges;
    A.cam = cam8.data(); A.freeOf = freeOf.data(); A.edgeObs = obs.data(); A.edgePose = ep.data(); A.edgePoint = ept.data();
    A.ptOff = ptOff.data(); A.poseOff = poseOff.data(); A.poseEdge = poseEdge.data(); A.edgeOf = edgeOf.data(); A.blockPose = blockPose.data();
    A.pose = pose.data(); A.pt = pt.data(); A.level = level.data(); A.chi2 = chi2.data(); A.lin = lin.data(); A.Y = Y.data();
    A.Hll = Hll.data(); A.bl = bl.data(); A.HllInv = HllInv.data(); A.Db = Db.data(); A.ptRho = ptRho.data(); A.ptScale = ptScale.data();
    A.ptAct = ptAct.data(); A.Hpp = Hpp.data(); A.bp = bp.data(); A.poseScale = poseScale.data(); A.poseAct = poseAct.data();
    A.S = S.data(); A.bs = bs.data(); A.xp = xp.data(); A.rec = &rec;
    be.erase = &erase;
    seen = false;
    // the flag is "raised before iteration stopBefore": an iteration begins with its linearisation
    auto stop = [&]() -> bool {
      const bool s = stopBefore >= 0 && be.linearised >= stopBefore;
      seen = seen || s;
      return s;
    };
    if (global) lba_schedule_global(be, stop, nIt, robust != 0, &run);
    else lba_schedule_local(be, stop, &run);
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < bestUs) bestUs = us;
  }
  std::vector<double> Tout(16 * (size_t)nLocal + 1);
  const double* hp = pose.data() + (size_t)be.cur * 8 * nT;
  for (int j = 0; j < nLocal; j++) lba_pose_to_Tcw(hp + 8 * (size_t)j, Tout.data() + 16 * (size_t)j);
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  const int32_t ints[8] = {run.rounds, seen ? 1 : 0, run.iterations[0], run.iterations[1], run.trials[0], run.trials[1], run.end[0], run.end[1]};
  bool ok = wr(g, Tout.data(), 16 * (size_t)nLocal) && wr(g, pt.data() + (size_t)be.cur * 3 * nP, 3 * nP) && wr(g, erase.data(), nE) &&
            wr(g, level.data(), nE) && wr(g, chi2.data(), nE) && wr(g, ints, 8) && wr(g, run.lambda, 2) && wr(g, run.chi2, 2);
  ok = std::fclose(g) == 0 && ok;
  if (!ok) return 2;
  std::printf("poses=%d points=%d edges=%d cpu_us=%.1f\n", (int)nT, nPoints, nEdges, bestUs);
  return 0;
}
