// orbfe_cpp::Initializer::Initialize / Reconstruct (include/orbfe_classes.hpp) on one scene file written by
// tests/test_gpu_initializer_reconstruct_cpp.py (tests/initializer_ref.py: write_scene): problem 0's pairs become two frames'
// keys (pair i = key i of both, every key matched, one unmatched reference key last), argv[2] holds the draws and argv[3..6] K.
// Calls Initialize, then FindModels + Reconstruct and, with the same operands, the C-ABI; prints whether the class returned the
// C-ABI's bytes and what it decided, for the Python test to compare with the restatement.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "initializer_scene.h"
#include "orbfe_classes.hpp"

int main(int argc, char** argv) {
  using namespace orbfe_cpp;
  if (argc < 7) return 2;
  InitScene S;
  if (!init_read_scene(argv[1], &S) || S.K < 1) { std::printf("error=cannot_read_scene\n"); return 2; }
  const InitSceneProblem& p = S.probs[0];
  std::vector<int32_t> draws((size_t)p.H * 8);
  {
    std::FILE* f = std::fopen(argv[2], "r");
    if (!f) { std::printf("error=cannot_read_draws\n"); return 2; }
    for (int32_t& d : draws)
      if (std::fscanf(f, "%d", &d) != 1) { std::printf("error=short_draws\n"); return 2; }
    std::fclose(f);
  }
  const float K4[4] = {(float)std::atof(argv[3]), (float)std::atof(argv[4]), (float)std::atof(argv[5]), (float)std::atof(argv[6])};
  try {
    std::vector<float> keys1, keys2;
    std::vector<int> vMatches12;
    for (int i = 0; i < p.n; i++) {
      keys1.insert(keys1.end(), {p.pairs[4 * (size_t)i], p.pairs[4 * (size_t)i + 1]});
      keys2.insert(keys2.end(), {p.pairs[4 * (size_t)i + 2], p.pairs[4 * (size_t)i + 3]});
      vMatches12.push_back(i);
    }
    keys1.insert(keys1.end(), {5.0f, 7.0f});  // an unmatched reference key, last
    vMatches12.push_back(-1);
    const Initializer init(keys1, p.sigma, p.H);
    double R21[9], t21[3];
    std::vector<float> vP3D;
    std::vector<bool> vbTriangulated;
    const bool ok = init.Initialize(keys2, vMatches12, draws, K4, R21, t21, vP3D, vbTriangulated);
    const Initializer::Models m = init.FindModels(keys2, vMatches12, draws);
    const Initializer::Reconstruction r = init.Reconstruct(m, K4);
    // the C-ABI with the same operands
    const size_t N = m.mvMatches12.size(), G = (size_t)r.nHyp;
    std::vector<uint32_t> words;
    InitializerReplay::pack(m.chooseH ? m.vbMatchesInliersH : m.vbMatchesInliersF, words);
    std::vector<double> R(G * 9), t(G * 3), cosSel(G), x3d(G * N * 3);
    std::vector<int32_t> nGood(G);
    std::vector<uint8_t> hypStatus(G), flags(G * N);
    uint8_t pst = 0;
    int32_t nInl = 0;
    check(orbfe_initializer_reconstruct(0, (int)N, m.pairs.data(), r.modelKind, m.chooseH ? m.H21 : m.F21, K4, p.sigma, words.data(),
                                        R.data(), t.data(), nGood.data(), cosSel.data(), hypStatus.data(), x3d.data(), flags.data(),
                                        &pst, &nInl), "reconstruct");
    auto same = [](const void* a, const void* b, size_t n) { return n == 0 || std::memcmp(a, b, n) == 0; };
    std::printf("bytes_equal %d %d %d %d %d %d %d %d %d\n", (int)same(R.data(), r.R.data(), G * 72), (int)same(t.data(), r.t.data(), G * 24),
                (int)same(cosSel.data(), r.cosSel.data(), G * 8), (int)same(x3d.data(), r.x3d.data(), G * N * 24),
                (int)(nGood == r.nGood), (int)(hypStatus == r.hypStatus), (int)(flags == r.pairFlags), (int)(pst == r.problemStatus),
                (int)(nInl == r.nInliers));
    std::printf("initialize_equals_reconstruct %d\n", (int)(ok == r.success && same(R21, r.R21, 72) && same(t21, r.t21, 24) &&
                                                              vP3D == r.vP3D && vbTriangulated == r.vbTriangulated));
    std::printf("decision %d %d %d %d %d %.17g\n", (int)ok, r.modelKind, r.best, (int)r.problemStatus, r.nInliers, r.parallax);
    std::printf("model"); for (int i = 0; i < 9; i++) std::printf(" %.17g", (m.chooseH ? m.H21 : m.F21)[i]); std::printf("\n");
    std::printf("mask"); for (bool b : (m.chooseH ? m.vbMatchesInliersH : m.vbMatchesInliersF)) std::printf(" %d", (int)b); std::printf("\n");
    std::printf("n_good"); for (int32_t v : r.nGood) std::printf(" %d", v); std::printf("\n");
    std::printf("R21"); for (double v : R21) std::printf(" %.17g", v); std::printf("\n");
    std::printf("t21"); for (double v : t21) std::printf(" %.17g", v); std::printf("\n");
    std::printf("vbTriangulated"); for (bool b : vbTriangulated) std::printf(" %d", (int)b); std::printf("\n");
    std::printf("vP3D"); for (float v : vP3D) std::printf(" %.9g", v); std::printf("\n");
  } catch (const std::exception& e) {
    std::printf("error=%s\n", e.what());
    return 1;
  }
  return 0;
}
