// csrc/tripoints_host.h as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_tri_points_host_san.py): orbfe_triangulated_points_select's definition on the engineered inputs of
// tests/tri_points_ref.py -- no neighbour, no created pair, one pair, a contested keypoint, an empty neighbour between two
// others, mnIds on both sides of key frame 1's, a scene 1e3 from the origin, octave 0 and n_levels - 1 -- on exactly-sized
// buffers, against a sequential walk written here; the capacity rule; every refused input.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "tripoints_host.h"

using namespace orbfe;

#define REQUIRE(c)                                                   \
  do {                                                               \
    if (!(c)) { std::printf("line %d: %s\n", __LINE__, #c); return 1; } \
  } while (0)

struct Pair { int k, i1, i2, st; };

struct Case {
  int n1 = 0, K = 0;
  int64_t id1 = 10;
  std::vector<int64_t> id2;
  std::vector<float> c1, c2, x3d, scale;
  std::vector<int32_t> match, octave;
  std::vector<uint8_t> status;
};

static Case make(int n1, const std::vector<int64_t>& ids, const std::vector<Pair>& pairs, unsigned seed, bool far) {
  Case c;
  c.n1 = n1; c.K = (int)ids.size(); c.id2 = ids;
  const float shift = far ? 1000.0f : 0.0f;
  c.c1 = {0.25f + shift, -0.5f - shift, 0.125f + shift};
  auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return (float)(seed >> 8 & 4095) / 4096.0f; };
  for (int k = 0; k < c.K; k++)
    for (int r = 0; r < 3; r++) c.c2.push_back(c.c1[(size_t)r] + 3.0f * rnd() - 1.5f);
  c.match.assign((size_t)c.K * n1, -1);
  c.status.assign((size_t)c.K * n1, 0);
  c.x3d.assign((size_t)c.K * n1 * 3, 0.0f);
  for (const Pair& p : pairs) {
    const size_t at = (size_t)p.k * n1 + p.i1;
    c.match[at] = p.i2; c.status[at] = (uint8_t)p.st;
    if (p.st == ORBFE_TRI_CREATED) {
      c.x3d[3 * at] = c.c1[0] + 4.0f * rnd() - 2.0f; c.x3d[3 * at + 1] = c.c1[1] + 4.0f * rnd() - 2.0f; c.x3d[3 * at + 2] = c.c1[2] + 2.0f + 5.0f * rnd();
    }
  }
  for (int i = 0; i < n1; i++) c.octave.push_back(i % 3 == 0 ? 0 : (i % 3 == 1 ? 7 : (int32_t)(rnd() * 8.0f) & 7));
  for (int l = 0; l < 8; l++) c.scale.push_back(l ? c.scale.back() * 1.2f : 1.0f);
  return c;
}

struct Result {
  const char* err;
  bool over;
  int32_t n;
  std::vector<int32_t> k, i1, i2;
  std::vector<float> pos, normal, lo, hi;
  std::vector<uint8_t> from;
};

// the call on buffers of exactly `capacity` entries
static Result run(const Case& c, int capacity) {
  Result r{};
  const size_t cap = (size_t)capacity;
  r.k.assign(cap, -7); r.i1.assign(cap, -7); r.i2.assign(cap, -7);
  r.pos.assign(3 * cap, -7.0f); r.normal.assign(3 * cap, -7.0f); r.lo.assign(cap, -7.0f); r.hi.assign(cap, -7.0f);
  r.from.assign(cap, 77);
  r.n = -1;
  r.err = triangulated_points_select(c.n1, c.K, c.match.data(), c.status.data(), c.x3d.data(), c.id1, c.id2.data(), c.c1.data(), c.c2.data(),
                                     c.octave.data(), c.scale.data(), 8, capacity, r.k.data(), r.i1.data(), r.i2.data(), r.pos.data(),
                                     r.normal.data(), r.lo.data(), r.hi.data(), r.from.data(), &r.n, &r.over);
  return r;
}

// the reference's two loops as they stand, with the masking of src/ORBmatcher.cc:800-803
static int check(const Case& c) {
  std::vector<char> has((size_t)c.n1, 0);
  std::vector<Pair> want;
  for (int k = 0; k < c.K; k++)
    for (int i1 = 0; i1 < c.n1; i1++) {
      const size_t at = (size_t)k * c.n1 + i1;
      if (c.match[at] < 0 || has[(size_t)i1] || c.status[at] != ORBFE_TRI_CREATED) continue;
      has[(size_t)i1] = 1;
      want.push_back({k, i1, c.match[at], 1});
    }
  const int m = (int)want.size();
  for (int cap : {m, m + 1}) {
    const Result r = run(c, cap);
    REQUIRE(!r.err && !r.over && r.n == m);
    for (int w = 0; w < m; w++) {
      const Pair& p = want[(size_t)w];
      REQUIRE(r.k[(size_t)w] == p.k && r.i1[(size_t)w] == p.i1 && r.i2[(size_t)w] == p.i2);
      const bool first2 = c.id2[(size_t)p.k] < c.id1;
      REQUIRE(r.from[(size_t)w] == (first2 ? 1 : 0));
      const size_t at = (size_t)p.k * c.n1 + p.i1;
      REQUIRE(std::memcmp(&r.pos[3 * (size_t)w], &c.x3d[3 * at], 12) == 0);
      // a unit-length sum of two unit vectors halves to a vector no longer than 1; the range scales by the two levels
      double len = 0.0;
      for (int q = 0; q < 3; q++) len += (double)r.normal[3 * (size_t)w + q] * r.normal[3 * (size_t)w + q];
      REQUIRE(len > 0.0 && len < 1.0 + 1e-5);
      double d = 0.0;
      for (int q = 0; q < 3; q++) d += ((double)c.x3d[3 * at + q] - c.c1[(size_t)q]) * ((double)c.x3d[3 * at + q] - c.c1[(size_t)q]);
      const double hi = std::sqrt(d) * c.scale[(size_t)c.octave[(size_t)p.i1]];
      REQUIRE(std::fabs(r.hi[(size_t)w] - hi) <= 1e-3 * hi && std::fabs(r.lo[(size_t)w] * c.scale[7] - r.hi[(size_t)w]) <= 1e-5 * hi);
    }
    if (cap == m + 1) REQUIRE(r.k[(size_t)m] == -7 && r.from[(size_t)m] == 77);  // nothing behind the last point
  }
  if (m > 0) {
    const Result r = run(c, m - 1);
    REQUIRE(r.err && r.over && r.n == m);
    for (int w = 0; w + 1 < m; w++) REQUIRE(r.k[(size_t)w] == -7 && r.lo[(size_t)w] == -7.0f);  // no array written
  }
  return 0;
}

int main() {
  const int C = ORBFE_TRI_CREATED, L = ORBFE_TRI_LOW_PARALLAX, R = ORBFE_TRI_REPROJ_1;
  std::vector<Pair> dense;
  for (int k = 0; k < 3; k++)
    for (int i1 = 0; i1 < 80; i1++)
      if ((i1 + 2 * k) % 4) dense.push_back({k, i1, (i1 * 7 + k) % 90, (i1 + k) % 3 ? C : L});
  std::vector<Pair> far;
  for (int k = 0; k < 2; k++)
    for (int i1 = k; i1 < 12; i1 += 2) far.push_back({k, i1, i1, C});
  const std::vector<Case> cases = {
      make(5, {}, {}, 1, false),
      make(6, {9, 2}, {{0, 1, 3, L}, {1, 1, 2, R}, {1, 4, 0, L}}, 2, false),
      make(4, {9}, {{0, 2, 5, C}}, 3, false),
      make(6, {11, 12, 13}, {{0, 3, 7, C}, {2, 3, 8, C}, {1, 3, 1, L}, {2, 5, 2, C}, {0, 0, 0, C}}, 4, false),
      make(5, {3, 30}, {{0, 2, 1, R}, {1, 2, 4, C}, {1, 0, 0, C}}, 5, false),
      make(8, {11, 12, 13}, {{0, 1, 1, C}, {0, 6, 2, C}, {1, 2, 3, L}, {2, 0, 4, C}, {2, 7, 5, C}}, 6, false),
      make(6, {3, 30}, {{0, 0, 2, C}, {1, 1, 3, C}, {0, 4, 0, C}, {1, 5, 1, C}}, 7, false),
      make(12, {3, 30}, far, 8, true),
      make(80, {3, 30, 11}, dense, 10, false),
      make(0, {3, 30}, {}, 11, false),
  };
  for (const Case& c : cases)
    if (check(c)) return 1;

  // the contested keypoint: the lower neighbour has it, the loser's i2 gets nothing
  {
    const Result r = run(cases[3], 6);
    REQUIRE(r.n == 3 && r.k[1] == 0 && r.i1[1] == 3 && r.i2[1] == 7 && r.k[2] == 2 && r.i1[2] == 5);
  }
  // refused inputs: nothing written
  {
    const Case& g = cases[3];
    auto refused = [&](const Case& c, int n1, int K, int levels, int capacity, bool nullOut = false, bool nullCount = false) {
      Result r{};
      const size_t cap = (size_t)(capacity > 0 ? capacity : 0);
      r.k.assign(cap, -7); r.i1.assign(cap, -7); r.i2.assign(cap, -7);
      r.pos.assign(3 * cap, -7.0f); r.normal.assign(3 * cap, -7.0f); r.lo.assign(cap, -7.0f); r.hi.assign(cap, -7.0f); r.from.assign(cap, 77);
      int32_t n = -1;
      bool over = true;
      const char* e = triangulated_points_select(n1, K, c.match.empty() ? nullptr : c.match.data(), c.status.empty() ? nullptr : c.status.data(),
                                                 c.x3d.empty() ? nullptr : c.x3d.data(), c.id1, c.id2.empty() ? nullptr : c.id2.data(),
                                                 c.c1.empty() ? nullptr : c.c1.data(), c.c2.empty() ? nullptr : c.c2.data(),
                                                 c.octave.empty() ? nullptr : c.octave.data(), c.scale.empty() ? nullptr : c.scale.data(), levels,
                                                 capacity, nullOut ? nullptr : r.k.data(), r.i1.data(), r.i2.data(), r.pos.data(), r.normal.data(),
                                                 r.lo.data(), r.hi.data(), r.from.data(), nullCount ? nullptr : &n, &over);
      for (size_t w = 0; w < cap; w++)
        if (r.k[w] != -7 || r.from[w] != 77) return false;
      return e != nullptr && !over;
    };
    REQUIRE(refused(g, -1, g.K, 8, 6) && refused(g, 16385, g.K, 8, 6) && refused(g, g.n1, -1, 8, 6) && refused(g, g.n1, 65, 8, 6));
    REQUIRE(refused(g, g.n1, g.K, 0, 6) && refused(g, g.n1, g.K, ORBFE_MAX_LEVELS + 1, 6) && refused(g, g.n1, g.K, 8, -1));
    REQUIRE(refused(g, g.n1, g.K, 8, 6, true) && refused(g, g.n1, g.K, 8, 6, false, true));
    Case c = g; c.match.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.status.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.x3d.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.id2.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.c1.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.c2.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.octave.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.scale.clear(); REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.id1 = -1; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.id2[1] = -1; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.id2[1] = c.id1; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.id2[2] = c.id2[0]; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.c1[1] = INFINITY; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.c2[7] = NAN; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.match[3] = -2; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.match[3] = 16384; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.match[2 * 6 + 5] = 8; REQUIRE(refused(c, g.n1, g.K, 8, 6));  // keypoint 8 of neighbour 2 named twice
    c = g; c.status[3] = 10; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.status[1] = (uint8_t)C; REQUIRE(refused(c, g.n1, g.K, 8, 6));  // a status without a match
    c = g; c.status[3] = 0; REQUIRE(refused(c, g.n1, g.K, 8, 6));           // a match without a status
    c = g; c.octave[3] = 8; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.octave[3] = -1; REQUIRE(refused(c, g.n1, g.K, 8, 6));
    c = g; c.octave[1] = 8; REQUIRE(!refused(c, g.n1, g.K, 8, 6));  // (matched, not created: its octave is not read)
  }
  std::printf("ok\n");
  return 0;
}
