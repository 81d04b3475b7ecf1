// Stand-alone program: the per-hypothesis arithmetic of csrc/sim3_math.h -- the very code k_sim3.hip compiles for the device
// -- and the checks and layout of csrc/sim3_host.h on the CPU, hypothesis by hypothesis and pair by pair as the kernel's
// waves and lanes do.  Reads a scene file (tests/sim3_ref.py: write_scene), writes n_inliers / status / sim3 / mask words /
// word_off, prints the single-thread time of the hypothesis loop.  Build with -ffp-contract=off (tests/test_sim3_math_cpu.py).
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "sim3_host.h"
#include "sim3_scene.h"

using namespace orbfe;

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: sim3_cpu scene result [repeats]\n"); return 2; }
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 1;
  Sim3Scene S;
  if (!sim3_read_scene(argv[1], &S)) { std::printf("cannot read %s\n", argv[1]); return 2; }
  const int K = S.K;
  std::vector<int32_t> pairOff(1, 0), hypOff(1, 0), triples, wordOff((size_t)K + 1);
  std::vector<float> x1, x2, e1, e2, cam1, cam2;
  for (const Sim3SceneCandidate& c : S.cands) {
    pairOff.push_back(pairOff.back() + c.n);
    hypOff.push_back(hypOff.back() + c.H);
    x1.insert(x1.end(), c.x1.begin(), c.x1.end()); x2.insert(x2.end(), c.x2.begin(), c.x2.end());
    for (int i = 0; i < c.n; i++) { e1.push_back((float)(9.210 * c.sigma2_1[i])); e2.push_back((float)(9.210 * c.sigma2_2[i])); }
    cam1.insert(cam1.end(), c.cam1, c.cam1 + 4); cam2.insert(cam2.end(), c.cam2, c.cam2 + 4);
    triples.insert(triples.end(), c.triples.begin(), c.triples.end());
  }
  const int N = pairOff.back(), H = hypOff.back();
  size_t W = 0;
  for (const Sim3SceneCandidate& c : S.cands) W += (size_t)c.H * (size_t)((c.n + 31) / 32);
  std::vector<int32_t> nInliers((size_t)H);
  std::vector<uint8_t> status((size_t)H);
  std::vector<float> sim3((size_t)H * 13);
  std::vector<uint32_t> words(W);
  if (const char* e = sim3_check(K, N, H, pairOff.data(), x1.data(), x2.data(), e1.data(), e2.data(), cam1.data(), cam2.data(),
                                 hypOff.data(), triples.data(), nInliers.data(), status.data(), sim3.data(), words.data(),
                                 wordOff.data())) {
    std::printf("refused: %s\n", e);
    return 1;
  }
  std::vector<Sim3Candidate> cands;
  std::vector<int32_t> hypCand;
  double bestUs = 1e300;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    sim3_layout(K, pairOff.data(), hypOff.data(), cam1.data(), cam2.data(), wordOff.data(), &cands, &hypCand);
    for (int h = 0; h < H; h++) {
      const Sim3Candidate& C = cands[hypCand[h]];
      float P1[3][3], P2[3][3];
      for (int j = 0; j < 3; j++)
        for (int i = 0; i < 3; i++) {
          const size_t p = (size_t)(C.pair0 + triples[3 * (size_t)h + j]) * 3;
          P1[j][i] = x1[p + i]; P2[j][i] = x2[p + i];
        }
      Sim3Transform T;
      sim3_compute(P1, P2, S.fixScale != 0, &T);
      const bool bad = sim3_nonfinite(T);
      uint32_t* w = words.data() + C.word0 + (size_t)(h - C.hyp0) * C.words;
      for (int i = 0; i < C.words; i++) w[i] = 0;
      int count = 0;
      for (int i = 0; i < C.nPairs && !bad; i++) {
        const size_t p = (size_t)(C.pair0 + i);
        if (sim3_is_inlier(T, C.K1, C.K2, &x1[3 * p], &x2[3 * p], e1[p], e2[p])) { w[i >> 5] |= 1u << (i & 31); count++; }
      }
      nInliers[h] = count;
      status[h] = (uint8_t)(bad ? kSim3Nonfinite : kSim3Ok);
      for (int i = 0; i < 9; i++) sim3[13 * (size_t)h + i] = (float)T.R[i];
      for (int i = 0; i < 3; i++) sim3[13 * (size_t)h + 9 + i] = (float)T.t[i];
      sim3[13 * (size_t)h + 12] = (float)T.s;
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < bestUs) bestUs = us;
  }
  if (!sim3_write_result(argv[2], nInliers, status, sim3, words, wordOff)) return 2;
  std::printf("hypotheses=%d cpu_us=%.1f\n", H, bestUs);
  return 0;
}
