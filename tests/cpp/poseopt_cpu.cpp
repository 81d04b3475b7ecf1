// Stand-alone program: the arithmetic of csrc/poseopt_math.h -- the very code k_poseopt.hip compiles for the device -- and the
// checks and packing of csrc/poseopt_host.h on the CPU, with the kernel's summation order: lane t of 256 adds edges t,
// t + 256, ... in ascending order, the 64 lanes of a wave combine as its __shfl_down tree does (offsets 32, 16, 8, 4, 2, 1;
// lane 0's total) and the four wave sums are added in wave order.  Reads a scene file (tests/pose_opt_check.py:
// write_scenes), writes per problem Tcw_out, n_inliers, the stats, outlier[] and edge_chi2[].  Build with -ffp-contract=off.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "poseopt_host.h"
#include "poseopt_math.h"

using namespace orbfe;

namespace {

constexpr int kT = kPoseOptThreads, kWaves = kT / 64;

template <typename T>
bool rd(std::FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <typename T>
bool wr(std::FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

// block_sum of k_poseopt.hip on the 256 lane values
double block_sum(double* v) {
  double s = 0.0;
  for (int w = 0; w < kWaves; w++) {
    double* l = v + 64 * w;
    for (int off = 32; off >= 1; off >>= 1)
      for (int i = 0; i < off; i++) l[i] = l[i] + l[i + off];
    s = w == 0 ? l[0] : s + l[0];
  }
  return s;
}

void load(const float* A, const float* B, int e, PoseOptEdge* E) {
  E->X[0] = (double)A[4 * e]; E->X[1] = (double)A[4 * e + 1]; E->X[2] = (double)A[4 * e + 2]; E->w = (double)A[4 * e + 3];
  E->u = (double)B[4 * e]; E->v = (double)B[4 * e + 1]; E->ur = (double)B[4 * e + 2];
}

// k_pose_optimize, one problem
void solve(const PoseOptProblem& pr, const float* A, const float* B, float deltaMono, float deltaStereo, PoseOptResult* res,
           uint8_t* level, double* chi2s) {
  const int n = pr.n;
  if (n < 3) { poseopt_result_untouched(pr, n, res); return; }
  for (int e = 0; e < n; e++) level[e] = 0;
  PoseOptCam C;
  for (int k = 0; k < 5; k++) C.K[k] = (double)pr.K5[k];
  C.deltaMono = (double)deltaMono; C.deltaStereo = (double)deltaStereo;
  G2oLM<6> lm;
  PoseOptPose start, est, P;
  int nActive = n, nBad = 0, rounds = 0;
  poseopt_pose_from_Tcw(pr.Tcw, &start);
  static double part[kPoseOptSums][kT];
  for (int rnd = 0; rnd < 4; rnd++) {
    const bool robust = rnd < 3;
    est = start;
    P = est;
    int cmd = nActive > 0 ? kG2oLMFull : kG2oLMDone;
    g2o_lm_begin(&lm, kPoseOptMaxIt);
    while (cmd != kG2oLMDone) {
      if (cmd == kG2oLMFull) {
        for (int t = 0; t < kT; t++) {
          double acc[kPoseOptSums];
          for (int k = 0; k < kPoseOptSums; k++) acc[k] = 0.0;
          for (int e = t; e < n; e += kT) {
            if (level[e] != 0) continue;
            PoseOptEdge E;
            load(A, B, e, &E);
            chi2s[e] = poseopt_edge_full(P, C, E, robust, acc);
          }
          for (int k = 0; k < kPoseOptSums; k++) part[k][t] = acc[k];
        }
        for (int k = 0; k < kPoseOptSums; k++) lm.S[k] = block_sum(part[k]);
        cmd = g2o_lm_after_full(&lm);
        poseopt_lm_propose(&lm, est, &P);
      } else {
        for (int t = 0; t < kT; t++) {
          double sum = 0.0;
          for (int e = t; e < n; e += kT) {
            if (level[e] != 0) continue;
            PoseOptEdge E;
            load(A, B, e, &E);
            chi2s[e] = poseopt_edge_trial(P, C, E, robust, &sum);
          }
          part[0][t] = sum;
        }
        cmd = g2o_lm_after_trial(&lm, block_sum(part[0]), &est, P, [&] { poseopt_lm_propose(&lm, est, &P); });
        if (cmd != kG2oLMTrial) P = est;
      }
    }
    for (int t = 0; t < kT; t++) {
      double cnt = 0.0;
      for (int e = t; e < n; e += kT) {
        PoseOptEdge E;
        load(A, B, e, &E);
        if (level[e] != 0) chi2s[e] = poseopt_edge_chi2(P, C, E);
        const bool bad = poseopt_is_outlier(chi2s[e], E);
        level[e] = bad ? 1 : 0;
        cnt = cnt + (bad ? 1.0 : 0.0);
      }
      part[0][t] = cnt;
    }
    nBad = (int)block_sum(part[0]);
    nActive = n - nBad;
    res->iterations[rnd] = lm.it; res->trials[rnd] = lm.trials; res->lambda[rnd] = lm.lam; res->chi2[rnd] = lm.cur;
    rounds = rnd + 1;
    if (n < 10) break;
  }
  for (int r = rounds; r < 4; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
  res->nInliers = n - nBad; res->nEdges = n; res->rounds = rounds; res->pad = 0;
  poseopt_pose_to_Tcw(est, res->Tcw);
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: poseopt_cpu scenes results\n"); return 2; }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  int32_t Q = 0;
  if (!rd(f, &Q, 1) || Q < 0) return 2;
  std::vector<int32_t> off(1, 0);
  std::vector<float> xw, u, v, ur, w, K5, Tcw;
  for (int p = 0; p < Q; p++) {
    int32_t n = 0;
    float k[5], T[16];
    if (!rd(f, &n, 1) || !rd(f, k, 5) || !rd(f, T, 16) || n < 0) return 2;
    const size_t at = (size_t)off.back();
    off.push_back(off.back() + n);
    xw.resize(3 * (at + n)); u.resize(at + n); v.resize(at + n); ur.resize(at + n); w.resize(at + n);
    if (!rd(f, xw.data() + 3 * at, 3 * (size_t)n) || !rd(f, u.data() + at, (size_t)n) || !rd(f, v.data() + at, (size_t)n) ||
        !rd(f, ur.data() + at, (size_t)n) || !rd(f, w.data() + at, (size_t)n)) return 2;
    K5.insert(K5.end(), k, k + 5);
    Tcw.insert(Tcw.end(), T, T + 16);
  }
  std::fclose(f);
  const int N = off.back();
  std::vector<float> out(16 * (size_t)Q + 1);
  std::vector<uint8_t> outlier((size_t)N + 1, 7);  // the flags a call starts from: untouched with fewer than 3 edges
  std::vector<double> chi2((size_t)N + 1, 0.0);
  std::vector<int32_t> nIn((size_t)Q + 1);
  if (const char* e = poseopt_check_batch(Q, off.data(), xw.data(), u.data(), v.data(), ur.data(), w.data(), K5.data(), Tcw.data(),
                                          out.data(), outlier.data(), nIn.data())) {
    std::printf("refused: %s\n", e);
    return 1;
  }
  std::vector<float> A(4 * (size_t)N + 4), B(4 * (size_t)N + 4);
  poseopt_pack_edges_a(A.data(), N, xw.data(), w.data());
  poseopt_pack_edges_b(B.data(), N, u.data(), v.data(), ur.data());
  const float deltaMono = (float)std::sqrt(5.991), deltaStereo = (float)std::sqrt(7.815);  // as poseopt.hip sets them
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  bool ok = true;
  std::vector<uint8_t> level;
  std::vector<double> c2;
  for (int p = 0; p < Q && ok; p++) {
    PoseOptProblem pr;
    pr.off = off[p]; pr.n = off[p + 1] - off[p]; pr.pad = 0.0f;
    for (int k = 0; k < 5; k++) pr.K5[k] = K5[5 * (size_t)p + k];
    for (int k = 0; k < 16; k++) pr.Tcw[k] = Tcw[16 * (size_t)p + k];
    const size_t at = (size_t)pr.off, n = (size_t)pr.n;
    level.assign(n + 1, 0); c2.assign(n + 1, 0.0);
    PoseOptResult r;
    solve(pr, A.data() + 4 * at, B.data() + 4 * at, deltaMono, deltaStereo, &r, level.data(), c2.data());
    if (pr.n >= 3) {  // as run_batch of poseopt.hip copies back
      for (size_t e = 0; e < n; e++) { outlier[at + e] = level[e]; chi2[at + e] = c2[e]; }
    }
    const int32_t ints[2] = {r.nInliers, r.rounds};
    ok = wr(g, r.Tcw, 16) && wr(g, ints, 2) && wr(g, r.iterations, 4) && wr(g, r.trials, 4) && wr(g, r.lambda, 4) &&
         wr(g, r.chi2, 4) && wr(g, outlier.data() + at, n) && wr(g, chi2.data() + at, n);
  }
  ok = std::fclose(g) == 0 && ok;
  if (!ok) return 2;
  std::printf("problems=%d edges=%d\n", Q, N);
  return 0;
}
