// The host loop of the four-trip path a caller had before orbfe_correct_loop_mappoints / orbfe_gba_update_mappoints, compiled
// for tools/loop_correct_latency.py: one CPU thread, -O2, flat arrays, no sanitizer.  Reads the arrays the tool wrote, runs
// the loop `reps` times on a copy of the positions, writes the new positions and the claimed list, prints the median in ms.
//   mode 0: CorrectLoop's point loop (src/LoopClosing.cc:558-587) without UpdateNormalAndDepth (the fourth trip does that)
//   mode 1: the map-point loop of RunGlobalBundleAdjustment (src/LoopClosing.cc:818-852)
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "loopcorrect_host.h"

using namespace orbfe;

template <typename T>
static std::vector<T> take(FILE* f, size_t n) {
  std::vector<T> v(n ? n : 1);
  if (n && std::fread(v.data(), sizeof(T), n, f) != n) { std::fprintf(stderr, "short read\n"); std::exit(2); }
  v.resize(n);
  return v;
}

int main(int argc, char** argv) {
  if (argc != 3) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  const std::vector<int32_t> hd = take<int32_t>(f, 5);  // mode, reps, K (or n_kf), width (or 0), P
  const int mode = hd[0], reps = hd[1], K = hd[2], W = hd[3], P = hd[4];
  std::vector<double> t;
  std::vector<float> out;
  std::vector<int32_t> list;
  if (mode == 0) {
    const std::vector<int32_t> rows = take<int32_t>(f, (size_t)K * W);
    const std::vector<uint8_t> skip = take<uint8_t>(f, (size_t)P);
    const std::vector<double> cor = take<double>(f, 8 * (size_t)K), non = take<double>(f, 8 * (size_t)K);
    const std::vector<float> xw = take<float>(f, 3 * (size_t)P);
    std::vector<int32_t> off((size_t)K + 1), ref((size_t)P);
    for (int k = 0; k <= K; k++) off[(size_t)k] = k * W;
    out.resize(3 * (size_t)P);
    for (int r = 0; r < reps; r++) {
      const auto t0 = std::chrono::steady_clock::now();
      if (correct_loop_points(K, cor.data(), non.data(), off.data(), rows.data(), P, xw.data(), skip.data(), out.data(), ref.data())) return 3;
      list.clear();
      for (int k = 0; k < K; k++)  // the slot list the fourth trip needs, in claim order
        for (int e = k * W; e < (k + 1) * W; e++)
          if (rows[(size_t)e] >= 0 && ref[(size_t)rows[(size_t)e]] == k) { list.push_back(rows[(size_t)e]); ref[(size_t)rows[(size_t)e]] = -2; }
      t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
  } else {
    const std::vector<uint8_t> bad = take<uint8_t>(f, (size_t)P), in = take<uint8_t>(f, (size_t)P);
    const std::vector<float> xw = take<float>(f, 3 * (size_t)P), pg = take<float>(f, 3 * (size_t)P);
    const std::vector<int32_t> ref = take<int32_t>(f, (size_t)P);
    const std::vector<uint8_t> reached = take<uint8_t>(f, (size_t)K);
    const std::vector<float> Tb = take<float>(f, 16 * (size_t)K), Tn = take<float>(f, 16 * (size_t)K);
    std::vector<uint8_t> moved((size_t)P);
    out.resize(3 * (size_t)P);
    for (int r = 0; r < reps; r++) {
      const auto t0 = std::chrono::steady_clock::now();
      if (gba_update_points(P, xw.data(), bad.data(), in.data(), pg.data(), ref.data(), K, reached.data(), Tb.data(), Tn.data(), out.data(),
                            moved.data())) return 3;
      t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    }
    list.assign(moved.begin(), moved.end());
  }
  std::fclose(f);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t n = (int32_t)list.size();
  std::fwrite(&n, 4, 1, o);
  std::fwrite(list.data(), 4, list.size(), o);
  std::fwrite(out.data(), 4, out.size(), o);
  std::fclose(o);
  std::sort(t.begin(), t.end());
  std::printf("%.4f\n", t[t.size() / 2]);
  return 0;
}
