// Stand-alone program with its own main: the host side of orbfe_initializer_reconstruct* -- csrc/initializer_host.h (recon_check,
// recon_layout), csrc/initializer_reconstruct_math.h (one hypothesis, as the kernel computes it) and
// include/orbfe_initializer_replay.hpp (the tails of ReconstructH / ReconstructF) -- built with -fsanitize=address,undefined and
// run directly (tests/test_initializer_reconstruct_host_san.py).  Every array is a std::vector exactly as long as the call says,
// so a read or write past an end is caught.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/orbfe_initializer_replay.hpp"
#include "initializer_host.h"

using namespace orbfe;
using orbfe_cpp::InitializerReplay;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("failed at line %d: %s\n", __LINE__, #c);          \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

struct Call {
  int K = 0, N = 0, W = 0;
  std::vector<int32_t> pairOff, wordOff, kind, hypOff, slotOff, nGood, nInliers;
  std::vector<float> pairs, K4, sigma;
  std::vector<double> model, R, t, cosSel, x3d;
  std::vector<uint32_t> words;
  std::vector<uint8_t> hypStatus, pairFlags, problemStatus;
  const char* check() const {
    return recon_check(K, N, W, pairOff.data(), pairs.data(), kind.data(), model.data(), K4.data(), sigma.data(), words.data(),
                       wordOff.data(), hypOff.data(), slotOff.data(), R.data(), t.data(), nGood.data(), cosSel.data(), hypStatus.data(),
                       x3d.data(), pairFlags.data(), problemStatus.data(), nInliers.data());
  }
};

// camera 2 = camera 1 moved by (0.3, 0, 0) and turned a little about y; K = 512 512 256 256
const double kRy = 0.05;
void project(double X, double Y, double Z, float p[4]) {
  const double c = std::cos(kRy), s = std::sin(kRy);
  const double x2 = c * X + s * Z + 0.3, y2 = Y, z2 = -s * X + c * Z;
  p[0] = (float)(512.0 * X / Z + 256.0); p[1] = (float)(512.0 * Y / Z + 256.0);
  p[2] = (float)(512.0 * x2 / z2 + 256.0); p[3] = (float)(512.0 * y2 / z2 + 256.0);
}

// problem 0: F, n general points; problem 1: H, n points of the plane Z = 4 (every third masked out); problem 2: F, no pairs
Call make(int n) {
  Call c;
  c.K = 3; c.N = 2 * n;
  const int w = (n + 31) / 32;
  c.W = 2 * w;
  c.pairOff = {0, n, 2 * n, 2 * n};
  c.wordOff = {0, w, 2 * w, 2 * w};
  c.kind = {kInitF, kInitH, kInitF};
  c.sigma = {1.0f, 1.0f, 2.0f};
  for (int k = 0; k < 3; k++) c.K4.insert(c.K4.end(), {512.0f, 512.0f, 256.0f, 256.0f});
  unsigned s = 2024u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (double)((s >> 8) & 0xFFFF) / 65536.0; };
  c.pairs.assign(8 * (size_t)n, 0.0f);
  c.words.assign(2 * (size_t)w, 0u);
  for (int i = 0; i < n; i++) {
    project(-1.5 + 3.0 * rnd(), -1.0 + 2.0 * rnd(), 3.0 + 4.0 * rnd(), &c.pairs[4 * (size_t)i]);
    project(-1.5 + 3.0 * rnd(), -1.0 + 2.0 * rnd(), 4.0, &c.pairs[4 * (size_t)(n + i)]);
    c.words[(size_t)(i >> 5)] |= 1u << (i & 31);
    if (i % 3) c.words[(size_t)(w + (i >> 5))] |= 1u << (i & 31);
  }
  const double cr = std::cos(kRy), sr = std::sin(kRy), tx = 0.3;
  const double R[9] = {cr, 0.0, sr, 0.0, 1.0, 0.0, -sr, 0.0, cr};
  const double Tx[9] = {0.0, 0.0, 0.0, 0.0, 0.0, -tx, 0.0, tx, 0.0};  // [t]x, t = (tx, 0, 0)
  const double Kd[9] = {512.0, 0.0, 256.0, 0.0, 512.0, 256.0, 0.0, 0.0, 1.0};
  const double Ki[9] = {1.0 / 512.0, 0.0, -0.5, 0.0, 1.0 / 512.0, -0.5, 0.0, 0.0, 1.0};
  double Kit[9], E[9], a[9], F[9], Hc[9], H[9];
  g2o_transpose3(Ki, Kit);
  g2o_mul3(Tx, R, E);
  g2o_mul3(Kit, E, a);
  g2o_mul3(a, Ki, F);
  for (int i = 0; i < 9; i++) Hc[i] = R[i];
  Hc[2] += tx / 4.0;  // R + t n^T / d, n = (0, 0, 1), d = 4
  g2o_mul3(Kd, Hc, a);
  g2o_mul3(a, Ki, H);
  c.model.insert(c.model.end(), F, F + 9);
  c.model.insert(c.model.end(), H, H + 9);
  c.model.insert(c.model.end(), F, F + 9);
  const size_t G = 4 + 8 + 4, S = (size_t)(4 + 8) * (size_t)n;
  c.hypOff.assign(4, 0); c.slotOff.assign(4, 0);
  c.R.assign(G * 9, 0.0); c.t.assign(G * 3, 0.0); c.cosSel.assign(G, 0.0); c.nGood.assign(G, 0); c.hypStatus.assign(G, 0);
  c.x3d.assign(S * 3, 0.0); c.pairFlags.assign(S, 0); c.problemStatus.assign(3, 0); c.nInliers.assign(3, 0);
  return c;
}

int run_all(Call& c) {
  std::vector<ReconProblem> probs;
  std::vector<int32_t> hypProb;
  recon_layout(c.K, c.pairOff.data(), c.kind.data(), c.model.data(), c.K4.data(), c.sigma.data(), c.wordOff.data(), c.hypOff.data(),
               c.slotOff.data(), &probs, &hypProb);
  REQUIRE(hypProb.size() == c.nGood.size() && (size_t)c.slotOff[c.K] == c.pairFlags.size() && (size_t)c.hypOff[c.K] == c.nGood.size());
  for (size_t g = 0; g < hypProb.size(); g++) {
    const size_t k = (size_t)hypProb[g];
    const ReconProblem& P = probs[k];
    const int hi = (int)g - P.hyp0;
    const size_t slot = (size_t)P.slot0 + (size_t)hi * (size_t)P.nPairs;
    std::vector<uint64_t> keys((size_t)P.nPairs);
    std::vector<double> x3d((size_t)P.nPairs * 3);  // exactly the hypothesis's share, copied out below
    std::vector<uint8_t> flags((size_t)P.nPairs);
    const std::vector<float> pairs(c.pairs.begin() + 4 * (size_t)P.pair0, c.pairs.begin() + 4 * (size_t)(P.pair0 + P.nPairs));
    const std::vector<uint32_t> words(c.words.begin() + P.word0, c.words.begin() + P.word0 + (P.nPairs + 31) / 32);
    bool deg;
    int32_t nInl;
    recon_hypothesis_host(P, pairs.data(), words.data(), hi, &c.R[9 * g], &c.t[3 * g], &c.nGood[g], &c.cosSel[g], &c.hypStatus[g],
                          x3d.data(), flags.data(), keys.data(), &deg, &nInl);
    if (!x3d.empty()) std::memcpy(&c.x3d[3 * slot], x3d.data(), x3d.size() * 8);
    if (!flags.empty()) std::memcpy(&c.pairFlags[slot], flags.data(), flags.size());
    if (hi == 0) { c.nInliers[k] = nInl; c.problemStatus[k] = (uint8_t)(deg ? kReconDegenerate : kReconProblemOk); }
  }
  return 0;
}

int self_test() {
  for (int n : {1, 32, 33, 64, 65, 120}) {
    Call c = make(n);
    REQUIRE(c.check() == nullptr);
    if (run_all(c)) return 1;
    REQUIRE(c.nInliers[0] == n && c.nInliers[1] == n - (n + 2) / 3 && c.nInliers[2] == 0);
    REQUIRE(c.problemStatus[0] == kReconProblemOk && c.problemStatus[1] == kReconProblemOk);
    int bestF = 0, bestH = 0;
    for (int g = 0; g < 4; g++) bestF = c.nGood[(size_t)g] > bestF ? c.nGood[(size_t)g] : bestF;
    for (int g = 4; g < 12; g++) bestH = c.nGood[(size_t)g] > bestH ? c.nGood[(size_t)g] : bestH;
    REQUIRE(bestF == n && bestH == c.nInliers[1]);  // the true motion accepts every inlier
    for (int g = 12; g < 16; g++) REQUIRE(c.nGood[(size_t)g] == 0 && c.cosSel[(size_t)g] == 0.0);
    double par[8];
    for (int g = 0; g < 4; g++) par[g] = InitializerReplay::parallax_degrees(c.nGood[(size_t)g], c.cosSel[(size_t)g]);
    const InitializerReplay::Outcome o = InitializerReplay::reconstruct_f(c.nInliers[0], c.nGood.data(), par);
    REQUIRE(o.success == (n > 50));
    if (o.success) {  // t = +(1, 0, 0), R the planted rotation
      REQUIRE(std::fabs(c.t[3 * (size_t)o.best] - 1.0) < 1e-6 && std::fabs(c.R[9 * (size_t)o.best + 2] - std::sin(kRy)) < 1e-6);
    }
    for (int g = 0; g < 8; g++) par[g] = InitializerReplay::parallax_degrees(c.nGood[(size_t)(4 + g)], c.cosSel[(size_t)(4 + g)]);
    (void)InitializerReplay::reconstruct_h(c.nInliers[1], c.nGood.data() + 4, par);
    // masked-out pairs of the H problem: zeros
    for (int g = 0; g < 8; g++)
      for (int i = 0; i < n; i += 3) REQUIRE(c.pairFlags[(size_t)c.slotOff[1] + (size_t)g * (size_t)n + (size_t)i] == 0);
  }
  {  // the replay on hand-made numbers
    const int f1[4] = {0, 100, 3, 0};
    const double p1[4] = {0.0, 2.0, 5.0, 0.0}, p2[4] = {0.0, 1.0, 5.0, 0.0};
    REQUIRE(InitializerReplay::reconstruct_f(100, f1, p1).best == 1 && !InitializerReplay::reconstruct_f(100, f1, p2).success);  // 1.0 is not > 1.0
    const int f2[4] = {100, 71, 0, 0}, f3[4] = {100, 70, 0, 0}, f4[4] = {100, 100, 0, 0};
    REQUIRE(!InitializerReplay::reconstruct_f(100, f2, p1).success);   // 71 > 0.7 * 100: two similar
    REQUIRE(!InitializerReplay::reconstruct_f(100, f3, p1).success);   // 70 is not similar, but parallax[0] == 0
    REQUIRE(!InitializerReplay::reconstruct_f(100, f4, p1).success);
    REQUIRE(!InitializerReplay::reconstruct_f(200, f1, p1).success);   // maxGood < int(0.9 N)
    const int h1[8] = {0, 5, 100, 74, 0, 0, 0, 0}, h2[8] = {0, 5, 100, 75, 0, 0, 0, 0}, h3[8] = {51, 0, 0, 0, 0, 0, 0, 0}, h4[8] = {50, 0, 0, 0, 0, 0, 0, 0};
    const double q1[8] = {0.0, 0.0, 1.0, 9.0, 0.0, 0.0, 0.0, 0.0}, q3[8] = {3.0, 0, 0, 0, 0, 0, 0, 0};
    REQUIRE(InitializerReplay::reconstruct_h(100, h1, q1).best == 2);  // 74 < 75, parallax 1.0 >= 1.0
    REQUIRE(!InitializerReplay::reconstruct_h(100, h2, q1).success);   // 75 is not < 75
    REQUIRE(InitializerReplay::reconstruct_h(56, h3, q3).success && !InitializerReplay::reconstruct_h(57, h3, q3).success);  // 51 > 50.4, not > 51.3
    REQUIRE(!InitializerReplay::reconstruct_h(40, h4, q3).success);    // 50 is not > minTriangulated
    REQUIRE(InitializerReplay::parallax_degrees(0, 0.5) == 0.0 && std::fabs(InitializerReplay::parallax_degrees(3, 0.5) - 60.0) < 1e-12);
    std::vector<uint32_t> wd;
    std::vector<bool> vb(33, false);
    vb[0] = vb[31] = vb[32] = true;
    InitializerReplay::pack(vb, wd);
    REQUIRE(wd.size() == 2 && wd[0] == 0x80000001u && wd[1] == 1u);
  }
  {  // an H model of a pure rotation: DEGENERATE, nothing evaluated
    Call c = make(40);
    const double I[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
    std::memcpy(&c.model[9], I, sizeof I);
    REQUIRE(c.check() == nullptr);
    if (run_all(c)) return 1;
    REQUIRE(c.problemStatus[1] == kReconDegenerate && c.nInliers[1] == 40 - 14);
    for (int g = 4; g < 12; g++) REQUIRE(c.nGood[(size_t)g] == 0 && c.R[9 * (size_t)g] == 0.0);
    for (size_t s = (size_t)c.slotOff[1]; s < (size_t)c.slotOff[2]; s++) REQUIRE(c.pairFlags[s] == 0 && c.x3d[3 * s] == 0.0);
  }
  {  // the order-preserving key
    const double v[6] = {-2.0, -0.0, 0.0, 0.5, 0.99998, 1.0};
    for (int i = 0; i < 5; i++) REQUIRE(recon_key(v[i]) < recon_key(v[i + 1]));
    for (double x : v) REQUIRE(recon_unkey(recon_key(x)) == x && recon_key(x) != kReconNoKey);
  }
  {  // refusals
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    Call g = make(33);
    REQUIRE(g.check() == nullptr);
    Call c = g; c.pairOff[0] = 1; REQUIRE(c.check() != nullptr);
    c = g; c.pairOff[1] = 70; REQUIRE(c.check() != nullptr);
    c = g; c.pairOff[3] = 65; REQUIRE(c.check() != nullptr);
    c = g; c.wordOff[0] = 1; REQUIRE(c.check() != nullptr);
    c = g; c.wordOff[1] = 1; REQUIRE(c.check() != nullptr);   // not ceil(33 / 32) words
    c = g; c.wordOff[3] = 5; REQUIRE(c.check() != nullptr);
    c = g; c.kind[1] = 2; REQUIRE(c.check() != nullptr);
    c = g; c.kind[0] = -1; REQUIRE(c.check() != nullptr);
    c = g; c.model[4] = nan; REQUIRE(c.check() != nullptr);
    c = g; c.model[17] = inf; REQUIRE(c.check() != nullptr);
    c = g; c.K4[2] = (float)nan; REQUIRE(c.check() != nullptr);
    c = g; c.K4[0] = 0.0f; REQUIRE(c.check() != nullptr);
    c = g; c.K4[5] = 0.0f; REQUIRE(c.check() != nullptr);
    c = g; c.sigma[0] = 0.0f; REQUIRE(c.check() != nullptr);
    c = g; c.sigma[2] = -1.0f; REQUIRE(c.check() != nullptr);
    c = g; c.sigma[1] = (float)inf; REQUIRE(c.check() != nullptr);
    c = g; c.K = -1; REQUIRE(c.check() != nullptr);
    c = g; c.K = 4097; REQUIRE(c.check() != nullptr);
    const int32_t zero = 0;
    REQUIRE(recon_check(0, 0, 0, &zero, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, &zero, &zero, &zero, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == nullptr);  // a call without problems is legal
    REQUIRE(recon_check(1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                        nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) != nullptr);
  }
  std::printf("ok\n");
  return 0;
}

}  // namespace

int main() { return self_test(); }
