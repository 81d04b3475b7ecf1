// Stand-alone program: the per-hypothesis arithmetic of csrc/initializer_math.h -- the very code k_initializer.hip compiles for
// the device -- and the checks and layout of csrc/initializer_host.h on the CPU, (set, model) by (set, model), row by row and
// pair by pair as the kernel's waves and lanes do.  Reads a scene file (tests/initializer_ref.py: write_scene), writes score /
// model / h12 / status / n_inliers / mask words / word_off, prints the single-thread time of the hypothesis loop.  Build with
// -ffp-contract=off (tests/test_initializer_math_cpu.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <initializer_list>
#include <vector>

#include "initializer_host.h"
#include "initializer_scene.h"

using namespace orbfe;

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: initializer_cpu scene result [repeats]\n"); return 2; }
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 1;
  InitScene S;
  if (!init_read_scene(argv[1], &S)) { std::printf("cannot read %s\n", argv[1]); return 2; }
  const InitOperands O(S);
  const int K = S.K, N = O.pairOff.back(), H = O.hypOff.back();
  std::vector<int32_t> wordOff((size_t)K + 1), nInliers((size_t)H * 2);
  std::vector<double> score((size_t)H * 2), model((size_t)H * 18), h12((size_t)H * 9);
  std::vector<uint8_t> status((size_t)H * 2);
  std::vector<uint32_t> words(O.words);
  if (const char* e = init_check(K, N, H, O.pairOff.data(), O.pairs.data(), O.T1.data(), O.T2.data(), O.sigma.data(), O.hypOff.data(),
                                 O.sets.data(), score.data(), status.data(), nInliers.data(), model.data(), h12.data(), words.data(),
                                 wordOff.data())) {
    std::printf("refused: %s\n", e);
    return 1;
  }
  std::vector<InitProblem> probs;
  std::vector<int32_t> hypProb;
  double bestUs = 1e300;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    init_layout(K, O.pairOff.data(), O.hypOff.data(), O.T1.data(), O.T2.data(), O.sigma.data(), wordOff.data(), &probs, &hypProb);
    for (int h = 0; h < H; h++) {
      const InitProblem& P = probs[hypProb[h]];
      for (int m = 0; m < 2; m++) {
        const size_t g = 2 * (size_t)h + m;
        double scratchH12[9];
        init_hypothesis_host(m, P, O.pairs.data() + 4 * (size_t)P.pair0, O.sets.data() + 8 * (size_t)h, &score[g], &status[g],
                             &nInliers[g], &model[9 * g], m == kInitH ? &h12[9 * (size_t)h] : scratchH12,
                             words.data() + P.word0 + ((size_t)(h - P.hyp0) * 2 + m) * P.words);
      }
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < bestUs) bestUs = us;
  }
  if (!init_write_result(argv[2], score, model, h12, status, nInliers, words, wordOff)) return 2;
  std::printf("sets=%d cpu_us=%.1f\n", H, bestUs);
  return 0;
}
