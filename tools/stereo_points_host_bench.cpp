// The host loop of the five-trip path a stereo caller had before orbfe_create_stereo_points, compiled for
// tools/stereo_points_latency.py: one CPU thread, -O2, flat arrays, no sanitizer.  Reads the arrays the tool wrote, runs
// the depth sort, the walk, Frame::UnprojectStereo, normal and range (csrc/stereopoints_host.h) and the gather of the new
// points' descriptors `reps` times, writes what the trips need, prints the median in ms.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "stereopoints_host.h"

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
  const std::vector<int32_t> hd = take<int32_t>(f, 4);  // n, reps, mode, n_levels
  const int n = hd[0], reps = hd[1], mode = hd[2], L = hd[3];
  const size_t N = (size_t)n;
  const std::vector<float> x = take<float>(f, N), y = take<float>(f, N), depth = take<float>(f, N);
  const std::vector<int32_t> octave = take<int32_t>(f, N);
  const std::vector<uint8_t> occupied = take<uint8_t>(f, N), stale = take<uint8_t>(f, N), desc = take<uint8_t>(f, 32 * N);
  const std::vector<uint8_t> poseBytes = take<uint8_t>(f, sizeof(orbfe_camera_pose));
  const std::vector<float> rest = take<float>(f, 4 + (size_t)L);  // th_depth, centre[3], scale[L]
  std::fclose(f);
  orbfe_camera_pose pose;
  std::memcpy(&pose, poseBytes.data(), sizeof(pose));
  std::vector<int32_t> idx(N);
  std::vector<float> pos(3 * N), normal(3 * N), lo(N), hi(N);
  std::vector<uint8_t> cleared(N), newDesc(32 * N);
  int32_t created = 0, walked = 0;
  std::vector<double> t;
  for (int r = 0; r < reps; r++) {
    const auto t0 = std::chrono::steady_clock::now();
    bool over = false;
    if (stereo_points_select(n, x.data(), y.data(), octave.data(), depth.data(), occupied.data(), stale.data(), &pose, rest[0], mode,
                             rest.data() + 4, L, rest.data() + 1, n, idx.data(), pos.data(), normal.data(), lo.data(), hi.data(),
                             cleared.data(), &created, &walked, &over))
      return 3;
    for (int j = 0; j < created; j++) std::memcpy(newDesc.data() + 32 * (size_t)j, desc.data() + 32 * (size_t)idx[(size_t)j], 32);
    t.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
  }
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const size_t m = (size_t)created;
  std::fwrite(&created, 4, 1, o);
  std::fwrite(idx.data(), 4, m, o);
  std::fwrite(pos.data(), 4, 3 * m, o);
  std::fwrite(normal.data(), 4, 3 * m, o);
  std::fwrite(lo.data(), 4, m, o);
  std::fwrite(hi.data(), 4, m, o);
  std::fwrite(newDesc.data(), 1, 32 * m, o);
  std::fclose(o);
  std::sort(t.begin(), t.end());
  std::printf("%.4f\n", t[t.size() / 2]);
  return 0;
}
