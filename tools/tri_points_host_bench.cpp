// The host loop a CreateNewMapPoints caller ran between orbfe_triangulate_matches_multi and its seven trips, compiled, for
// tools/tri_points_latency.py: the replay of the neighbours in order (keep pair (k, i1) when its status is CREATED and
// winner[i1] == k) and the gathers of positions, key frame 1's descriptor rows, octaves and the index lists the trips take.
// Reads one binary file -- n1, K, reps as int32; match12 [K * n1] int32; status [K * n1] uint8; winner [n1] int32; x3d
// [K * n1 * 3] float; octave1 [n1] int32; desc1 [n1 * 32] uint8 -- and prints the median time of `reps` runs in ms.  One
// CPU thread, -O2, no sanitizer.
#include <algorithm>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

template <typename T>
static bool take(FILE* f, std::vector<T>* v, size_t n) {
  v->resize(n);
  return n == 0 || std::fread(v->data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t head[3];
  if (std::fread(head, 4, 3, f) != 3) return 2;
  const size_t n1 = (size_t)head[0], K = (size_t)head[1];
  const int reps = head[2];
  std::vector<int32_t> match, winner, octave;
  std::vector<uint8_t> status, desc;
  std::vector<float> x3d;
  if (!take(f, &match, K * n1) || !take(f, &status, K * n1) || !take(f, &winner, n1) || !take(f, &x3d, K * n1 * 3) || !take(f, &octave, n1) ||
      !take(f, &desc, n1 * 32))
    return 2;
  std::fclose(f);
  std::vector<double> ms;
  size_t made = 0;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<int32_t> ck, kf2;
    std::vector<uint16_t> i1s, i2s;
    std::vector<uint8_t> oct, d;
    std::vector<float> pos;
    for (size_t k = 0; k < K; k++)
      for (size_t i1 = 0; i1 < n1; i1++) {
        const size_t at = k * n1 + i1;
        if (status[at] != 1 || winner[i1] != (int32_t)k) continue;
        ck.push_back((int32_t)k);
        i1s.push_back((uint16_t)i1);
        i2s.push_back((uint16_t)match[at]);
        oct.push_back((uint8_t)octave[i1]);
        pos.insert(pos.end(), x3d.begin() + 3 * at, x3d.begin() + 3 * at + 3);
        d.insert(d.end(), desc.begin() + 32 * i1, desc.begin() + 32 * i1 + 32);
      }
    const auto t1 = std::chrono::steady_clock::now();
    ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    made = ck.size() + (d.size() + pos.size() + i1s.size() + i2s.size() + oct.size()) * 0;  // (the results are used)
  }
  std::sort(ms.begin(), ms.end());
  std::printf("%.6f %zu\n", ms[ms.size() / 2], made);
  return 0;
}
