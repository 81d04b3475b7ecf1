// The scene file of the Initializer tests (tests/initializer_ref.py: write_scene / read_result), shared by initializer_cpu.cpp
// and test_initializer.cpp: whitespace-separated numbers, floats as their float32 and doubles as their float64 bit patterns
// in hex.
#pragma once
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct InitSceneProblem {
  int n = 0, H = 0;
  float sigma = 1.0f;
  double T1[4], T2[4];
  std::vector<float> pairs;
  std::vector<int32_t> sets;
};
struct InitScene {
  int K = 0;
  std::vector<InitSceneProblem> probs;
};

inline bool init_read_floats(std::FILE* f, float* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    unsigned bits;
    if (std::fscanf(f, "%x", &bits) != 1) return false;
    const uint32_t b = bits;
    std::memcpy(out + i, &b, 4);
  }
  return true;
}
inline bool init_read_doubles(std::FILE* f, double* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    uint64_t b;
    if (std::fscanf(f, "%" SCNx64, &b) != 1) return false;
    std::memcpy(out + i, &b, 8);
  }
  return true;
}

inline bool init_read_scene(const char* path, InitScene* S) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  bool ok = std::fscanf(f, "%d", &S->K) == 1 && S->K >= 0;
  S->probs.resize(ok ? (size_t)S->K : 0);
  for (int k = 0; ok && k < S->K; k++) {
    InitSceneProblem& p = S->probs[k];
    ok = std::fscanf(f, "%d %d", &p.n, &p.H) == 2 && p.n >= 0 && p.H >= 0;
    if (!ok) break;
    p.pairs.resize(4 * (size_t)p.n);
    p.sets.resize(8 * (size_t)p.H);
    ok = init_read_floats(f, &p.sigma, 1) && init_read_doubles(f, p.T1, 4) && init_read_doubles(f, p.T2, 4) &&
         init_read_floats(f, p.pairs.data(), p.pairs.size());
    for (size_t i = 0; ok && i < p.sets.size(); i++) ok = std::fscanf(f, "%d", &p.sets[i]) == 1;
  }
  std::fclose(f);
  return ok;
}

// the flat arrays of orbfe_initializer_ransac_multi
struct InitOperands {
  std::vector<int32_t> pairOff{0}, hypOff{0}, sets;
  std::vector<float> pairs, sigma;
  std::vector<double> T1, T2;
  size_t words = 0;
  explicit InitOperands(const InitScene& S) {
    for (const InitSceneProblem& p : S.probs) {
      pairOff.push_back(pairOff.back() + p.n);
      hypOff.push_back(hypOff.back() + p.H);
      pairs.insert(pairs.end(), p.pairs.begin(), p.pairs.end());
      sets.insert(sets.end(), p.sets.begin(), p.sets.end());
      sigma.push_back(p.sigma);
      T1.insert(T1.end(), p.T1, p.T1 + 4);
      T2.insert(T2.end(), p.T2, p.T2 + 4);
      words += 2 * (size_t)p.H * (size_t)((p.n + 31) / 32);
    }
  }
};

// score, model, h12 (bit patterns), status, n_inliers, the number of mask words, the words, then `rest`
inline bool init_write_result(const char* path, const std::vector<double>& score, const std::vector<double>& model,
                              const std::vector<double>& h12, const std::vector<uint8_t>& status,
                              const std::vector<int32_t>& nInliers, const std::vector<uint32_t>& words,
                              const std::vector<int32_t>& rest) {
  std::FILE* f = std::fopen(path, "w");
  if (!f) return false;
  for (const std::vector<double>* a : {&score, &model, &h12})
    for (double v : *a) {
      uint64_t b;
      std::memcpy(&b, &v, 8);
      std::fprintf(f, "%016" PRIx64 " ", b);
    }
  for (uint8_t v : status) std::fprintf(f, "%d ", (int)v);
  for (int32_t v : nInliers) std::fprintf(f, "%d ", v);
  std::fprintf(f, "%zu ", words.size());
  for (uint32_t v : words) std::fprintf(f, "%08x ", v);
  for (int32_t v : rest) std::fprintf(f, "%d ", v);
  std::fprintf(f, "\n");
  return std::fclose(f) == 0;
}
