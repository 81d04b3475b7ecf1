// Stand-alone program with its own main: the host side of orbfe_initializer_ransac* -- csrc/initializer_host.h (checks, layout,
// Normalize, the selection of the sets), csrc/initializer_math.h (one hypothesis, as the kernel computes it) and
// include/orbfe_initializer_replay.hpp (the scans and the choice) -- built with -fsanitize=address,undefined and run directly
// (tests/test_initializer_host_san.py).  Every array is a std::vector exactly as long as the call says, so a read or write past
// an end is caught.
//   (no argument)      a two-problem call with an empty problem, every refusal, the replay; prints "ok"
//   sets n H           draws [H * 8] on stdin -> the sets, or "refused"
//   normalize n        x y pairs on stdin -> T as four %.17g numbers, or "refused"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "../../include/orbfe_initializer_replay.hpp"
#include "initializer_host.h"

using namespace orbfe;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) {                                                      \
      std::printf("failed at line %d: %s\n", __LINE__, #c);          \
      return 1;                                                      \
    }                                                                \
  } while (0)

namespace {

struct Call {
  int K = 0, N = 0, H = 0;
  std::vector<int32_t> pairOff, hypOff, sets, wordOff, nInliers;
  std::vector<float> pairs, sigma;
  std::vector<double> T1, T2, score, model, h12;
  std::vector<uint8_t> status;
  std::vector<uint32_t> words;
  const char* check() const {
    return init_check(K, N, H, pairOff.data(), pairs.data(), T1.data(), T2.data(), sigma.data(), hypOff.data(), sets.data(),
                      score.data(), status.data(), nInliers.data(), model.data(), h12.data(), words.data(), wordOff.data());
  }
};

// problem 0: n pairs of a plane seen from two places (x2 = H x1) and H sets; problem 1: empty
Call make(int n, int H) {
  Call c;
  c.K = 2; c.N = n; c.H = H;
  c.pairOff = {0, n, n}; c.hypOff = {0, H, H};
  c.wordOff.assign(3, 0);
  c.sigma = {1.0f, 2.0f};
  unsigned s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)((s >> 8) & 0xFFFF) / 65536.0f; };
  const double G[9] = {1.02, 0.03, 12.0, -0.02, 0.98, -7.0, 1e-5, -2e-5, 1.0};
  for (int i = 0; i < n; i++) {
    const float x = 40.0f + 560.0f * rnd(), y = 30.0f + 420.0f * rnd();
    const double w = G[6] * x + G[7] * y + G[8];
    c.pairs.insert(c.pairs.end(), {x, y, (float)((G[0] * x + G[1] * y + G[2]) / w), (float)((G[3] * x + G[4] * y + G[5]) / w)});
  }
  c.T1.assign(8, 0.0); c.T2.assign(8, 0.0);
  std::vector<float> k1, k2;
  for (int i = 0; i < n; i++) { k1.insert(k1.end(), {c.pairs[4 * i], c.pairs[4 * i + 1]}); k2.insert(k2.end(), {c.pairs[4 * i + 2], c.pairs[4 * i + 3]}); }
  init_normalize(n, k1.data(), c.T1.data());
  init_normalize(n, k2.data(), c.T2.data());
  c.T1[4] = c.T1[5] = c.T2[4] = c.T2[5] = 1.0;  // (the empty problem's)
  std::vector<int32_t> draws((size_t)H * 8);
  for (int h = 0; h < H; h++)
    for (int j = 0; j < 8; j++) draws[8 * (size_t)h + j] = (int32_t)(rnd() * (float)(n - j)) % (n - j);
  c.sets.assign((size_t)H * 8, 0);
  init_sets_from_draws(n, H, draws.data(), c.sets.data());
  const size_t w = (size_t)((n + 31) / 32);
  c.score.assign((size_t)H * 2, 0.0); c.model.assign((size_t)H * 18, 0.0); c.h12.assign((size_t)H * 9, 0.0);
  c.status.assign((size_t)H * 2, 0); c.nInliers.assign((size_t)H * 2, 0); c.words.assign(2 * (size_t)H * w, 0u);
  return c;
}

int run_all(Call& c) {
  std::vector<InitProblem> probs;
  std::vector<int32_t> hypProb;
  init_layout(c.K, c.pairOff.data(), c.hypOff.data(), c.T1.data(), c.T2.data(), c.sigma.data(), c.wordOff.data(), &probs, &hypProb);
  REQUIRE((int)hypProb.size() == c.H && (size_t)c.wordOff[c.K] == c.words.size());
  for (int h = 0; h < c.H; h++) {
    const InitProblem& P = probs[(size_t)hypProb[(size_t)h]];
    for (int m = 0; m < 2; m++) {
      const size_t g = 2 * (size_t)h + (size_t)m;
      double none[9];
      init_hypothesis_host(m, P, c.pairs.data() + 4 * (size_t)P.pair0, c.sets.data() + 8 * (size_t)h, &c.score[g], &c.status[g],
                           &c.nInliers[g], &c.model[9 * g], m == kInitH ? &c.h12[9 * (size_t)h] : none,
                           c.words.data() + P.word0 + ((size_t)(h - P.hyp0) * 2 + (size_t)m) * (size_t)P.words);
    }
  }
  return 0;
}

int self_test() {
  for (int n : {8, 31, 32, 33, 64, 65, 129}) {
    Call c = make(n, 5);
    REQUIRE(c.check() == nullptr);
    if (run_all(c)) return 1;
    for (int h = 0; h < c.H; h++) {  // a plane: every H hypothesis finds every pair
      REQUIRE(c.status[2 * (size_t)h] == kInitOk && c.nInliers[2 * (size_t)h] == n);
    }
    const orbfe_cpp::InitializerReplay::Pick pH = orbfe_cpp::InitializerReplay::scan(c.H, 0, c.score.data());
    const orbfe_cpp::InitializerReplay::Pick pF = orbfe_cpp::InitializerReplay::scan(c.H, 1, c.score.data());
    REQUIRE(pH.best >= 0 && pH.score > 0.0);
    std::vector<bool> vb;
    orbfe_cpp::InitializerReplay::inliers(n, pH.best, 0, c.words.data(), vb);
    REQUIRE((int)vb.size() == n);
    for (int i = 0; i < n; i++) REQUIRE(vb[(size_t)i]);
    orbfe_cpp::InitializerReplay::inliers(n, -1, 1, c.words.data(), vb);
    for (int i = 0; i < n; i++) REQUIRE(!vb[(size_t)i]);
    const double RH = orbfe_cpp::InitializerReplay::ratio(pH.score, pF.score);
    REQUIRE(RH > 0.0 && RH <= 1.0);
  }
  {  // the replay on hand-made scores: the first of equal bests, NaN never, nothing above 0
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const std::vector<double> sc = {1.0, 0.0, nan, nan, 3.0, 0.0, 3.0, -1.0, 2.0, 0.0};
    const auto a = orbfe_cpp::InitializerReplay::scan(5, 0, sc.data()), b = orbfe_cpp::InitializerReplay::scan(5, 1, sc.data());
    REQUIRE(a.best == 2 && a.score == 3.0 && b.best == -1 && b.score == 0.0);
    REQUIRE(orbfe_cpp::InitializerReplay::choose_h(orbfe_cpp::InitializerReplay::ratio(3.0, 0.0)));
    REQUIRE(!orbfe_cpp::InitializerReplay::choose_h(orbfe_cpp::InitializerReplay::ratio(0.0, 0.0)));  // NaN
    REQUIRE(!orbfe_cpp::InitializerReplay::choose_h(orbfe_cpp::InitializerReplay::ratio(2.0, 3.0)));  // 0.4 is not > 0.40
  }
  {  // eight indices, one pair of coordinates, the means at it: H singular, H12 zero, the score NaN
    Call c = make(40, 1);
    for (int i = 1; i < 8; i++) std::memcpy(&c.pairs[4 * (size_t)i], &c.pairs[0], 16);
    for (int j = 0; j < 8; j++) c.sets[(size_t)j] = j;
    c.T1[2] = c.pairs[0]; c.T1[3] = c.pairs[1]; c.T2[2] = c.pairs[2]; c.T2[3] = c.pairs[3];
    REQUIRE(c.check() == nullptr);
    if (run_all(c)) return 1;
    REQUIRE(c.status[0] == kInitNonfinite && c.nInliers[0] == 0 && std::isnan(c.score[0]));
    for (int i = 0; i < 9; i++) REQUIRE(c.h12[(size_t)i] == 0.0);
    for (uint32_t w : c.words) REQUIRE(w == 0u || c.status[1] == kInitOk);
    REQUIRE(orbfe_cpp::InitializerReplay::scan(1, 0, c.score.data()).best == -1);
  }
  {  // refusals
    Call g = make(20, 3);
    REQUIRE(g.check() == nullptr);
    Call c = g; c.pairOff[1] = 21; REQUIRE(c.check() != nullptr);                // not monotone
    c = g; c.pairOff[2] = 19; REQUIRE(c.check() != nullptr);                     // does not end at N
    c = g; c.pairOff[0] = 1; REQUIRE(c.check() != nullptr);
    c = g; c.hypOff[2] = 4; REQUIRE(c.check() != nullptr);
    c = g; c.hypOff[0] = 1; REQUIRE(c.check() != nullptr);
    c = g; c.sets[7] = 20; REQUIRE(c.check() != nullptr);                        // outside [0, n_k)
    c = g; c.sets[3] = -1; REQUIRE(c.check() != nullptr);
    c = g; c.sets[15] = c.sets[8]; REQUIRE(c.check() != nullptr);                // repeated
    c = g; c.T1[1] = std::numeric_limits<double>::infinity(); REQUIRE(c.check() != nullptr);
    c = g; c.T2[6] = std::numeric_limits<double>::quiet_NaN(); REQUIRE(c.check() != nullptr);
    c = g; c.sigma[0] = 0.0f; REQUIRE(c.check() != nullptr);
    c = g; c.sigma[1] = -1.0f; REQUIRE(c.check() != nullptr);
    c = g; c.sigma[0] = std::numeric_limits<float>::quiet_NaN(); REQUIRE(c.check() != nullptr);
    c = make(7, 0); c.H = 1; c.hypOff = {0, 1, 1}; c.sets = {0, 1, 2, 3, 4, 5, 6, 0};  // fewer than 8 pairs with a set
    c.score.assign(2, 0.0); c.model.assign(18, 0.0); c.h12.assign(9, 0.0); c.status.assign(2, 0); c.nInliers.assign(2, 0); c.words.assign(2, 0u);
    REQUIRE(c.check() != nullptr);
    c = make(0, 0);  // a call of two empty problems is legal
    REQUIRE(c.check() == nullptr);
    REQUIRE(init_check(1, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                       nullptr, nullptr, nullptr) != nullptr);
    double T[4];
    REQUIRE(!init_normalize(0, nullptr, T) && !init_normalize(3, nullptr, T));
    int32_t s8[8];
    const int32_t d8[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    REQUIRE(!init_sets_from_draws(7, 1, d8, s8) && !init_sets_from_draws(8, 1, nullptr, s8) && init_sets_from_draws(7, 0, nullptr, nullptr));
  }
  std::printf("ok\n");
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc == 1) return self_test();
  if (argc == 4 && !std::strcmp(argv[1], "sets")) {
    const int n = std::atoi(argv[2]), H = std::atoi(argv[3]);
    std::vector<int32_t> draws((size_t)H * 8), sets((size_t)H * 8);
    for (int32_t& d : draws)
      if (std::scanf("%d", &d) != 1) return 2;
    if (!init_sets_from_draws(n, H, draws.data(), sets.data())) { std::printf("refused\n"); return 0; }
    for (int32_t v : sets) std::printf("%d ", v);
    std::printf("\n");
    return 0;
  }
  if (argc == 3 && !std::strcmp(argv[1], "normalize")) {
    const int n = std::atoi(argv[2]);
    std::vector<float> xy((size_t)(n > 0 ? n : 0) * 2);
    for (float& v : xy)
      if (std::scanf("%f", &v) != 1) return 2;
    double T[4];
    if (!init_normalize(n, xy.data(), T)) { std::printf("refused\n"); return 0; }
    std::printf("%.17g %.17g %.17g %.17g\n", T[0], T[1], T[2], T[3]);
    return 0;
  }
  std::printf("usage: initializer_host_san [sets n H | normalize n]\n");
  return 2;
}
