// The scene file of the Initializer reconstruct tests (tests/initializer_reconstruct_ref.py: write_scene / read_result), shared
// by initializer_reconstruct_cpu.cpp and test_initializer_reconstruct.cpp: whitespace-separated numbers, floats as their
// float32 and doubles as their float64 bit patterns in hex.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "initializer_scene.h"  // init_read_floats / init_read_doubles

struct ReconSceneProblem {
  int n = 0, kind = 0;
  float sigma = 1.0f, K4[4];
  double model[9];
  std::vector<float> pairs;
  std::vector<uint32_t> words;
};
struct ReconScene {
  int K = 0;
  std::vector<ReconSceneProblem> probs;
};

inline bool recon_read_scene(const char* path, ReconScene* S) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  bool ok = std::fscanf(f, "%d", &S->K) == 1 && S->K >= 0;
  S->probs.resize(ok ? (size_t)S->K : 0);
  for (int k = 0; ok && k < S->K; k++) {
    ReconSceneProblem& p = S->probs[(size_t)k];
    ok = std::fscanf(f, "%d %d", &p.n, &p.kind) == 2 && p.n >= 0;
    if (!ok) break;
    p.pairs.resize(4 * (size_t)p.n);
    p.words.resize((size_t)((p.n + 31) / 32));
    ok = init_read_floats(f, &p.sigma, 1) && init_read_floats(f, p.K4, 4) && init_read_doubles(f, p.model, 9) &&
         init_read_floats(f, p.pairs.data(), p.pairs.size());
    for (size_t i = 0; ok && i < p.words.size(); i++) {
      unsigned w;
      ok = std::fscanf(f, "%x", &w) == 1;
      p.words[i] = w;
    }
  }
  std::fclose(f);
  return ok;
}

// the flat arrays of orbfe_initializer_reconstruct_multi and outputs of the right sizes
struct ReconOperands {
  std::vector<int32_t> pairOff{0}, wordOff{0}, kind, hypOff, slotOff, nGood, nInliers;
  std::vector<float> pairs, sigma, K4;
  std::vector<double> model, R, t, cosSel, x3d;
  std::vector<uint32_t> words;
  std::vector<uint8_t> hypStatus, pairFlags, problemStatus;
  size_t G = 0, S = 0;
  explicit ReconOperands(const ReconScene& sc) {
    for (const ReconSceneProblem& p : sc.probs) {
      pairOff.push_back(pairOff.back() + p.n);
      wordOff.push_back(wordOff.back() + (int32_t)p.words.size());
      kind.push_back(p.kind);
      pairs.insert(pairs.end(), p.pairs.begin(), p.pairs.end());
      words.insert(words.end(), p.words.begin(), p.words.end());
      sigma.push_back(p.sigma);
      K4.insert(K4.end(), p.K4, p.K4 + 4);
      model.insert(model.end(), p.model, p.model + 9);
      const size_t g = p.kind == 0 ? 8 : 4;
      G += g;
      S += g * (size_t)p.n;
    }
    const size_t K = sc.probs.size();
    hypOff.assign(K + 1, 0); slotOff.assign(K + 1, 0);
    R.assign(G * 9, 0.0); t.assign(G * 3, 0.0); cosSel.assign(G, 0.0); nGood.assign(G, 0); hypStatus.assign(G, 0);
    x3d.assign(S * 3, 0.0); pairFlags.assign(S, 0); problemStatus.assign(K, 0); nInliers.assign(K, 0);
  }
};

inline bool recon_write_result(const char* path, const ReconOperands& o) {
  std::FILE* f = std::fopen(path, "w");
  if (!f) return false;
  auto ints = [&](const std::vector<int32_t>& a) { for (int32_t v : a) std::fprintf(f, "%d ", v); };
  auto bytes = [&](const std::vector<uint8_t>& a) { for (uint8_t v : a) std::fprintf(f, "%d ", (int)v); };
  auto dbl = [&](const std::vector<double>& a) {
    for (double v : a) {
      uint64_t b;
      std::memcpy(&b, &v, 8);
      std::fprintf(f, "%016" PRIx64 " ", b);
    }
  };
  ints(o.hypOff); ints(o.slotOff); dbl(o.R); dbl(o.t); ints(o.nGood); dbl(o.cosSel); bytes(o.hypStatus); dbl(o.x3d);
  bytes(o.pairFlags); bytes(o.problemStatus); ints(o.nInliers);
  std::fprintf(f, "\n");
  return std::fclose(f) == 0;
}
