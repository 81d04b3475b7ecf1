// Stand-alone program: the arithmetic of csrc/optsim3_math.h -- the very code k_optsim3.hip compiles for the device -- and the
// checks and packing of csrc/optsim3_host.h on the CPU, with the kernel's summation order: 64 lane-strided partial sums
// (lane l adds pairs l, l + 64, ... in ascending order, e12 then e21 of a pair) combined as the wave's __shfl_down tree does
// (offsets 32, 16, 8, 4, 2, 1; lane 0's total).  Reads a scene file (tests/test_optimize_sim3_math_cpu.py: write_scenes),
// writes per problem the result record, bad[], chi2_12[], chi2_21[], and prints the single-thread time of the best repeat.
// Build with -ffp-contract=off.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "optsim3_host.h"

using namespace orbfe;

namespace {

constexpr int kLanes = 64;

template <typename T>
bool rd(std::FILE* f, T* p, size_t n) { return n == 0 || std::fread(p, sizeof(T), n, f) == n; }
template <typename T>
bool wr(std::FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }

// lane 0's total of the wave's tree: v[l] += v[l + off] for off = 32 .. 1
double tree(double* v) {
  for (int off = 32; off >= 1; off >>= 1)
    for (int l = 0; l < off; l++) v[l] = v[l] + v[l + off];
  return v[0];
}

void solve(const OptSim3Problem& pr, const float* A, const float* B, const float* C, OptSim3Result* res, uint8_t* bad,
           double* chi12, double* chi21) {
  const int n = pr.n;
  const OptSim3Cam K1 = {(double)pr.cam1[0], (double)pr.cam1[1], (double)pr.cam1[2], (double)pr.cam1[3]};
  const OptSim3Cam K2 = {(double)pr.cam2[0], (double)pr.cam2[1], (double)pr.cam2[2], (double)pr.cam2[3]};
  const double delta = (double)pr.delta;
  const bool fixScale = pr.fixScale != 0;
  G2oLM<7> lm;
  OptSim3Vertex vx;
  vx.fixScale = fixScale;
  optsim3_from_record(pr.sim3, &vx.est);
  int rounds = 0, nBad = 0, nIn = 0, maxIt = 5;
  bool early = true;
  for (int r = 0; r < 2; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
  if (n > 0) {
    for (int i = 0; i < n; i++) bad[i] = 0;
    for (int rnd = 0; rnd < 2; rnd++) {
      g2o_lm_begin(&lm, maxIt);
      int cmd = kG2oLMFull;
      while (cmd != kG2oLMDone) {
        OptSim3Eval E;
        if (cmd == kG2oLMFull) {
          optsim3_eval_at(vx.est, &E);
          static double part[kOptSim3Sums][kLanes];
          for (int lane = 0; lane < kLanes; lane++) {
            double acc[kOptSim3Sums];
            for (int k = 0; k < kOptSim3Sums; k++) acc[k] = 0.0;
            for (int i = lane; i < n; i += kLanes) {
              if (bad[i] != 0) continue;
              OptSim3Pair p;
              optsim3_unpack(A + 4 * (size_t)i, B + 4 * (size_t)i, C + 4 * (size_t)i, &p);
              optsim3_pair_full(E, K1, K2, p, delta, fixScale, acc, &chi12[i], &chi21[i]);
            }
            for (int k = 0; k < kOptSim3Sums; k++) part[k][lane] = acc[k];
          }
          for (int k = 0; k < kOptSim3Sums; k++) lm.S[k] = tree(part[k]);
          cmd = g2o_lm_after_full(&lm);
          optsim3_lm_propose(&lm, &vx);
        } else {
          optsim3_eval_at(vx.trial, &E);
          double part[kLanes];
          for (int lane = 0; lane < kLanes; lane++) {
            double sum = 0.0;
            for (int i = lane; i < n; i += kLanes) {
              if (bad[i] != 0) continue;
              OptSim3Pair p;
              optsim3_unpack(A + 4 * (size_t)i, B + 4 * (size_t)i, C + 4 * (size_t)i, &p);
              optsim3_pair_trial(E, K1, K2, p, delta, &sum, &chi12[i], &chi21[i]);
            }
            part[lane] = sum;
          }
          cmd = g2o_lm_after_trial(&lm, tree(part), &vx.est, vx.trial, [&] { optsim3_lm_propose(&lm, &vx); });
        }
      }
      int erased = 0, kept = 0;
      for (int i = 0; i < n; i++) {
        if (bad[i] != 0) continue;
        if (optsim3_is_bad(chi12[i], chi21[i], pr.th2)) { bad[i] = (uint8_t)(rnd + 1); erased++; }
        else kept++;
      }
      res->iterations[rnd] = lm.it; res->trials[rnd] = lm.trials; res->lambda[rnd] = lm.lam; res->chi2[rnd] = lm.cur;
      rounds = rnd + 1;
      if (rnd == 0) {
        nBad = erased;
        maxIt = nBad > 0 ? 10 : 5;
        if (n - nBad < kOptSim3MinPairs) break;
      } else {
        nIn = kept;
        early = false;
      }
    }
  }
  if (early) optsim3_from_record(pr.sim3, &vx.est);
  for (int k = 0; k < 4; k++) res->sim3[k] = vx.est.q[k];
  for (int k = 0; k < 3; k++) res->sim3[4 + k] = vx.est.t[k];
  res->sim3[7] = vx.est.s;
  res->nIn = nIn; res->nBad = nBad; res->rounds = rounds; res->pad = 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: optsim3_cpu scenes results [repeats]\n"); return 2; }
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 1;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  int32_t K = 0;
  if (!rd(f, &K, 1) || K < 0) return 2;
  std::vector<int32_t> off(1, 0);
  std::vector<float> x1, x2, o1, o2, w1, w2, cam1, cam2, sim3, th2;
  std::vector<uint8_t> fix;
  for (int p = 0; p < K; p++) {
    int32_t n = 0, fx = 0;
    float t = 0, c[8], s[13];
    if (!rd(f, &n, 1) || !rd(f, &fx, 1) || !rd(f, &t, 1) || !rd(f, c, 8) || !rd(f, s, 13) || n < 0) return 2;
    const size_t at = (size_t)off.back();
    off.push_back(off.back() + n);
    x1.resize(3 * (at + n)); x2.resize(3 * (at + n)); o1.resize(2 * (at + n)); o2.resize(2 * (at + n));
    w1.resize(at + n); w2.resize(at + n);
    if (!rd(f, x1.data() + 3 * at, 3 * (size_t)n) || !rd(f, x2.data() + 3 * at, 3 * (size_t)n) ||
        !rd(f, o1.data() + 2 * at, 2 * (size_t)n) || !rd(f, o2.data() + 2 * at, 2 * (size_t)n) ||
        !rd(f, w1.data() + at, (size_t)n) || !rd(f, w2.data() + at, (size_t)n)) return 2;
    cam1.insert(cam1.end(), c, c + 4); cam2.insert(cam2.end(), c + 4, c + 8);
    sim3.insert(sim3.end(), s, s + 13);
    th2.push_back(t); fix.push_back((uint8_t)fx);
  }
  std::fclose(f);
  const int N = off.back();
  std::vector<double> out((size_t)8 * K + 1), c12((size_t)N + 1), c21((size_t)N + 1);
  std::vector<uint8_t> bad((size_t)N + 1);
  std::vector<int32_t> nIn((size_t)K + 1);
  if (const char* e = optsim3_check_multi(K, off.data(), x1.data(), x2.data(), o1.data(), o2.data(), w1.data(), w2.data(),
                                          cam1.data(), cam2.data(), sim3.data(), th2.data(), fix.data(), out.data(), bad.data(),
                                          nIn.data())) {
    std::printf("refused: %s\n", e);
    return 1;
  }
  std::vector<OptSim3Problem> prob((size_t)K);
  std::vector<OptSim3Result> res((size_t)K);
  std::vector<float> A(4 * (size_t)N + 4), B(4 * (size_t)N + 4), C(4 * (size_t)N + 4);
  double bestUs = 1e300;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    optsim3_pack_problems(prob.data(), K, off.data(), cam1.data(), cam2.data(), sim3.data(), th2.data(), fix.data());
    optsim3_pack_pairs_a(A.data(), N, x1.data(), w1.data());
    optsim3_pack_pairs_b(B.data(), N, x2.data(), w2.data());
    optsim3_pack_pairs_c(C.data(), N, o1.data(), o2.data());
    for (int p = 0; p < K; p++) {
      const size_t at = (size_t)prob[p].off;
      solve(prob[p], A.data() + 4 * at, B.data() + 4 * at, C.data() + 4 * at, &res[p], bad.data() + at, c12.data() + at,
            c21.data() + at);
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < bestUs) bestUs = us;
  }
  std::FILE* g = std::fopen(argv[2], "wb");
  if (!g) return 2;
  bool ok = true;
  for (int p = 0; p < K && ok; p++) {
    const OptSim3Result& r = res[p];
    const int32_t ints[7] = {r.nIn, r.nBad, r.rounds, r.iterations[0], r.iterations[1], r.trials[0], r.trials[1]};
    const size_t at = (size_t)prob[p].off, n = (size_t)prob[p].n;
    ok = wr(g, r.sim3, 8) && wr(g, r.lambda, 2) && wr(g, r.chi2, 2) && wr(g, ints, 7) && wr(g, bad.data() + at, n) &&
         wr(g, c12.data() + at, n) && wr(g, c21.data() + at, n);
  }
  ok = std::fclose(g) == 0 && ok;
  if (!ok) return 2;
  std::printf("problems=%d pairs=%d cpu_us=%.1f\n", K, N, bestUs);
  return 0;
}
