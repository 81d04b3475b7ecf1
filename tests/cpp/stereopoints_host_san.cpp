// csrc/stereopoints_host.h as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_stereo_points_host_san.py): the selection on engineered frames -- sizes 0, 1, 63, 64, 65, 130, ties, the stop
// at j = 100, depths 0 / -1 / NaN / +inf -- in all three modes on exactly-sized buffers, the capacity rule, and every
// refused input.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <vector>

#include "stereopoints_host.h"

using namespace orbfe;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

struct Frame {
  std::vector<float> x, y, depth;
  std::vector<int32_t> octave;
  std::vector<uint8_t> occupied, stale;
};

static Frame make(const std::vector<float>& depth, unsigned seed) {
  Frame f;
  const size_t n = depth.size();
  f.depth = depth;
  for (size_t i = 0; i < n; i++) {
    seed = seed * 1664525u + 1013904223u;
    f.x.push_back(5.0f + (float)(seed >> 8 & 1023) * 0.7f);
    f.y.push_back(5.0f + (float)(seed >> 18 & 511) * 0.9f);
    f.octave.push_back((int32_t)(seed >> 28 & 7));
    f.occupied.push_back((seed >> 4 & 3) == 0);
    f.stale.push_back(!f.occupied.back() && (seed >> 6 & 3) == 0);
  }
  return f;
}

static orbfe_camera_pose pose_of() {
  orbfe_camera_pose p{};
  const float R[9] = {0.36f, 0.48f, -0.8f, -0.8f, 0.6f, 0.0f, 0.48f, 0.64f, 0.6f};
  for (int k = 0; k < 9; k++) p.Rcw[k] = R[k];
  p.Ow[0] = 1000.0f; p.Ow[1] = -1000.0f; p.Ow[2] = 1000.0f;
  p.fx = 458.654f; p.fy = 457.296f; p.cx = 367.215f; p.cy = 248.375f; p.mbf = 40.0f;
  p.n_levels = 8;
  return p;
}

// the call on buffers of exactly `capacity` entries; returns the status text (NULL: done)
struct Result {
  const char* err;
  bool over;
  int32_t created, walked;
  std::vector<int32_t> idx;
  std::vector<uint8_t> cleared;
};
static Result run(const Frame& f, const orbfe_camera_pose& p, int mode, int capacity, const std::vector<float>& scale) {
  Result r{};
  const int n = (int)f.depth.size();
  const size_t c = (size_t)capacity;
  std::vector<int32_t> idx(c);
  std::vector<float> pos(3 * c), normal(3 * c), lo(c), hi(c);
  std::vector<uint8_t> cleared((size_t)n);
  const float centre[3] = {p.Ow[0] + 0.03125f, p.Ow[1], p.Ow[2] - 0.0625f};
  r.err = stereo_points_select(n, f.x.data(), f.y.data(), f.octave.data(), f.depth.data(), f.occupied.data(), f.stale.data(), &p, 10.0f, mode,
                               scale.data(), (int)scale.size(), centre, capacity, idx.data(), pos.data(), normal.data(), lo.data(), hi.data(),
                               cleared.data(), &r.created, &r.walked, &r.over);
  if (!r.err) idx.resize((size_t)r.created);
  r.idx = idx;
  r.cleared = cleared;
  return r;
}

int main() {
  std::vector<float> scale;
  for (int k = 0; k < 8; k++) scale.push_back(std::pow(1.2f, (float)k));
  const orbfe_camera_pose p = pose_of();
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  std::vector<std::vector<float>> depths;
  for (int n : {0, 1, 63, 64, 65, 130}) {
    std::vector<float> d;
    for (int i = 0; i < n; i++) d.push_back(i % 4 == 3 ? -1.0f : 0.5f + (float)((i * 37) % 59) * 0.5f);
    depths.push_back(d);
  }
  depths.push_back({2, 1, 2, 1, 3, 2, 1, 3, 2, 1, 2, 3});
  depths.push_back({0.0f, -1.0f, nan, inf, 2.0f, -0.0f, 1.0f, nan, 3.0f, -inf});
  std::vector<float> stop;
  for (int i = 0; i < 100; i++) stop.push_back(1.0f + 0.08f * (float)((i * 7) % 100));
  stop.insert(stop.begin() + 40, {15.0f, 10.0f, 17.0f});  // 100 close, one equal to th, two far
  depths.push_back(stop);
  unsigned seed = 9;
  for (const std::vector<float>& d : depths) {
    const Frame f = make(d, seed++);
    int candidates = 0;
    for (float z : d) candidates += z > 0 ? 1 : 0;
    for (int mode : {ORBFE_STEREO_ALL, ORBFE_STEREO_KEYFRAME, ORBFE_STEREO_TEMPORAL}) {
      const Result full = run(f, p, mode, (int)d.size(), scale);
      REQUIRE(!full.err && !full.over && full.walked <= candidates && full.created <= full.walked);
      if (mode == ORBFE_STEREO_ALL) REQUIRE(full.created == candidates && full.walked == candidates);
      if (candidates <= kStereoMinWalk) REQUIRE(full.walked == candidates);
      for (size_t i = 0; i < d.size(); i++) REQUIRE(!full.cleared[i] || (mode == ORBFE_STEREO_KEYFRAME && f.stale[i]));
      const Result exact = run(f, p, mode, full.created, scale);  // buffers of exactly the created count
      REQUIRE(!exact.err && exact.idx == full.idx);
      if (full.created > 0) {
        const Result small = run(f, p, mode, full.created - 1, scale);
        REQUIRE(small.err && small.over && small.created == full.created && small.walked == full.walked);
      }
    }
  }
  {  // 100 close + th + two far: the walk passes z == th and stops at the first far one, j = 101
    const Frame f = make(stop, 77);
    Frame g = f;
    g.occupied.assign(g.occupied.size(), 0);
    g.stale.assign(g.stale.size(), 0);
    const Result r = run(g, p, ORBFE_STEREO_KEYFRAME, 103, scale);
    REQUIRE(!r.err && r.walked == 102 && r.created == 102 && r.idx[100] == 41 && r.idx[101] == 40);
  }
  // refused inputs: nothing is written (the counts keep their sentinels where the check comes before them)
  {
    const Frame f = make(depths[4], 5);
    auto refused = [&](const Frame& fr, orbfe_camera_pose q, int mode, const std::vector<float>& sc) {
      const Result r = run(fr, q, mode, (int)fr.depth.size(), sc);
      return r.err != nullptr && !r.over;
    };
    REQUIRE(!refused(f, p, ORBFE_STEREO_KEYFRAME, scale));
    REQUIRE(refused(f, p, 3, scale));
    Frame b = f;
    b.octave[7] = 8;
    REQUIRE(refused(b, p, ORBFE_STEREO_ALL, scale));
    b = f;
    b.occupied[3] = b.stale[3] = 1;
    REQUIRE(refused(b, p, ORBFE_STEREO_KEYFRAME, scale) && !refused(b, p, ORBFE_STEREO_ALL, scale));
    orbfe_camera_pose q = p;
    q.fx = 0.0f;
    REQUIRE(refused(f, q, ORBFE_STEREO_ALL, scale));
    q = p;
    q.Rcw[2] = nan;
    REQUIRE(refused(f, q, ORBFE_STEREO_ALL, scale));
    q = p;
    q.Ow[1] = inf;
    REQUIRE(refused(f, q, ORBFE_STEREO_ALL, scale));
    REQUIRE(refused(f, p, ORBFE_STEREO_ALL, std::vector<float>(257, 1.0f)));
    Frame big = make(std::vector<float>(16385, 0.0f), 1);
    REQUIRE(refused(big, p, ORBFE_STEREO_ALL, scale));
  }
  {  // the close-point counts
    const std::vector<float> z = {0.0f, 10.0f, 9.5f, 1e-30f, nan, inf, -1.0f, 3.0f};
    const std::vector<uint8_t> has = {1, 1, 1, 0, 1, 1, 1, 1}, out = {0, 0, 0, 0, 0, 0, 0, 1};
    int32_t t = -1, u = -1;
    REQUIRE(!count_close_points((int)z.size(), z.data(), has.data(), out.data(), 10.0f, &t, &u) && t == 1 && u == 2);
    REQUIRE(count_close_points(-1, nullptr, nullptr, nullptr, 10.0f, &t, &u) != nullptr);
    REQUIRE(!count_close_points(0, nullptr, nullptr, nullptr, 10.0f, &t, &u) && t == 0 && u == 0);
  }
  std::printf("ok\n");
  return 0;
}
