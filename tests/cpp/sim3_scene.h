// The scene file of the Sim3 tests (tests/sim3_ref.py: write_scene / read_result), shared by sim3_cpu.cpp and test_sim3.cpp:
// whitespace-separated numbers, floats as their float32 bit patterns in hex.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

struct Sim3SceneCandidate {
  int n = 0, H = 0, N1 = 0;
  float cam1[4], cam2[4];
  std::vector<float> x1, x2, sigma2_1, sigma2_2;
  std::vector<int32_t> indices1, triples;
};
struct Sim3Scene {
  int K = 0, fixScale = 0;
  std::vector<Sim3SceneCandidate> cands;
};

inline bool sim3_read_floats(std::FILE* f, float* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    unsigned bits;
    if (std::fscanf(f, "%x", &bits) != 1) return false;
    const uint32_t b = bits;
    std::memcpy(out + i, &b, 4);
  }
  return true;
}
inline bool sim3_read_ints(std::FILE* f, std::vector<int32_t>* out, size_t n) {
  out->resize(n);
  for (size_t i = 0; i < n; i++)
    if (std::fscanf(f, "%d", &(*out)[i]) != 1) return false;
  return true;
}

inline bool sim3_read_scene(const char* path, Sim3Scene* S) {
  std::FILE* f = std::fopen(path, "r");
  if (!f) return false;
  bool ok = std::fscanf(f, "%d %d", &S->K, &S->fixScale) == 2 && S->K >= 0;
  S->cands.resize(ok ? (size_t)S->K : 0);
  for (int k = 0; ok && k < S->K; k++) {
    Sim3SceneCandidate& c = S->cands[k];
    ok = std::fscanf(f, "%d %d %d", &c.n, &c.H, &c.N1) == 3 && c.n >= 0 && c.H >= 0;
    if (!ok) break;
    const size_t n = (size_t)c.n;
    c.x1.resize(3 * n); c.x2.resize(3 * n); c.sigma2_1.resize(n); c.sigma2_2.resize(n);
    ok = sim3_read_floats(f, c.cam1, 4) && sim3_read_floats(f, c.cam2, 4) && sim3_read_floats(f, c.x1.data(), 3 * n) &&
         sim3_read_floats(f, c.x2.data(), 3 * n) && sim3_read_floats(f, c.sigma2_1.data(), n) &&
         sim3_read_floats(f, c.sigma2_2.data(), n) && sim3_read_ints(f, &c.indices1, n) && sim3_read_ints(f, &c.triples, 3 * (size_t)c.H);
  }
  std::fclose(f);
  return ok;
}

// n_inliers, status, sim3 (bit patterns), the number of mask words, the words, then `rest`
inline bool sim3_write_result(const char* path, const std::vector<int32_t>& nInliers, const std::vector<uint8_t>& status,
                              const std::vector<float>& sim3, const std::vector<uint32_t>& words, const std::vector<int32_t>& rest) {
  std::FILE* f = std::fopen(path, "w");
  if (!f) return false;
  for (int32_t v : nInliers) std::fprintf(f, "%d ", v);
  for (uint8_t v : status) std::fprintf(f, "%d ", (int)v);
  for (float v : sim3) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    std::fprintf(f, "%08x ", b);
  }
  std::fprintf(f, "%zu ", words.size());
  for (uint32_t v : words) std::fprintf(f, "%08x ", v);
  for (int32_t v : rest) std::fprintf(f, "%d ", v);
  std::fprintf(f, "\n");
  return std::fclose(f) == 0;
}
