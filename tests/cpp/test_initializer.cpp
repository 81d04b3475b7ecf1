// orbfe_cpp::Initializer (include/orbfe_classes.hpp) on one scene file written by tests/test_gpu_initializer_cpp.py
// (tests/initializer_ref.py: write_scene): problem 0's pairs become two frames' keys (pair i = key i of both, every key
// matched), its sets the draws' outcome.  Calls FindModels and, with the same operands, the C-ABI; prints whether the class
// returned the C-ABI's bytes and what it chose, for the Python test to compare with the restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "initializer_scene.h"
#include "orbfe_classes.hpp"

int main(int argc, char** argv) {
  using namespace orbfe_cpp;
  if (argc < 3) return 2;
  InitScene S;
  if (!init_read_scene(argv[1], &S) || S.K < 1) { std::printf("error=cannot_read_scene\n"); return 2; }
  const InitSceneProblem& p = S.probs[0];
  // the draws that give the scene's sets: argv[2] holds them
  std::vector<int32_t> draws((size_t)p.H * 8);
  {
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) { std::printf("error=cannot_read_draws\n"); return 2; }
    for (int32_t& d : draws)
      if (std::fscanf(f, "%d", &d) != 1) { std::printf("error=short_draws\n"); return 2; }
    std::fclose(f);
  }
  try {
    std::vector<float> keys1, keys2;
    std::vector<int> vMatches12;
    for (int i = 0; i < p.n; i++) {
      keys1.insert(keys1.end(), {p.pairs[4 * (size_t)i], p.pairs[4 * (size_t)i + 1]});
      keys2.insert(keys2.end(), {p.pairs[4 * (size_t)i + 2], p.pairs[4 * (size_t)i + 3]});
      vMatches12.push_back(i);
    }
    keys1.insert(keys1.end(), {5.0f, 7.0f});  // an unmatched reference key, last: mvMatches12 skips it
    vMatches12.push_back(-1);
    const Initializer init(keys1, p.sigma, p.H);
    const Initializer::Models m = init.FindModels(keys2, vMatches12, draws);
    std::printf("matches %zu sets_equal %d\n", m.mvMatches12.size(), (int)(m.mvSets == p.sets));
    // the C-ABI with the same operands
    double T1[4], T2[4];
    check(orbfe_initializer_normalize((int)(keys1.size() / 2), keys1.data(), T1), "normalize");
    check(orbfe_initializer_normalize((int)(keys2.size() / 2), keys2.data(), T2), "normalize");
    const size_t w = (size_t)((p.n + 31) / 32), H = (size_t)p.H;
    std::vector<double> score(H * 2), model(H * 18), h12(H * 9);
    std::vector<uint8_t> status(H * 2);
    std::vector<int32_t> nInl(H * 2);
    std::vector<uint32_t> words(H * 2 * w);
    check(orbfe_initializer_ransac(0, p.n, p.pairs.data(), T1, T2, p.sigma, p.H, p.sets.data(), score.data(), status.data(),
                                   nInl.data(), model.data(), h12.data(), words.data()), "ransac");
    auto same = [](const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; };
    std::printf("bytes_equal %d %d %d %d %d %d\n", (int)same(score.data(), m.score.data(), H * 16),
                (int)same(model.data(), m.model.data(), H * 144), (int)same(h12.data(), m.h12.data(), H * 72),
                (int)(status == m.status), (int)(nInl == m.nInliers), (int)(words == m.words));
    std::printf("T %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", T1[0], T1[1], T1[2], T1[3], T2[0], T2[1], T2[2], T2[3]);
    std::printf("pick %d %d %.17g %.17g %.17g %d\n", m.bestH, m.bestF, m.SH, m.SF, m.RH, (int)m.chooseH);
    std::printf("H21"); for (double v : m.H21) std::printf(" %.17g", v); std::printf("\n");
    std::printf("F21"); for (double v : m.F21) std::printf(" %.17g", v); std::printf("\n");
    std::printf("maskH"); for (bool b : m.vbMatchesInliersH) std::printf(" %d", (int)b); std::printf("\n");
    std::printf("maskF"); for (bool b : m.vbMatchesInliersF) std::printf(" %d", (int)b); std::printf("\n");
    bool threw = false;
    try { init.FindModels(keys2, vMatches12, std::vector<int32_t>(3)); } catch (const std::invalid_argument&) { threw = true; }
    std::printf("short_draws_throw %d\n", (int)threw);
  } catch (const std::exception& e) {
    std::printf("error=%s\n", e.what());
    return 1;
  }
  return 0;
}
