// The argument checks of orbfe_project_sim3 / orbfe_search_by_sim3_mappoints_multi that need no device
// (csrc/mappoints_host.h: sim3_check_legs, sim3_check_search) as a stand-alone program, built with the address and
// undefined-behaviour sanitizers by tests/test_sim3_search_host.py: every array is exactly as long as the call says, so a check
// that reads past one is reported.
#include <cstdio>
#include <cstring>
#include <vector>

#include "mappoints_host.h"

using namespace orbfe;

static int failures = 0;
#define EXPECT(cond)                                             \
  do {                                                           \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); failures++; } \
  } while (0)

static bool says(const char* e, const char* part) { return e && std::strstr(e, part); }

static std::vector<orbfe_sim3_leg> legs_of(int n, int levels) {
  std::vector<orbfe_sim3_leg> l((size_t)n);
  for (auto& x : l) { std::memset(&x, 0, sizeof x); x.n_levels = levels; }
  return l;
}

int main() {
  const int cap = 100;
  std::vector<int32_t> slot = {0, 99, -1, 5, 42, -1};
  std::vector<int32_t> off3 = {0, 4, 4, 6};  // three legs, the middle one empty
  auto legs = legs_of(3, 8);

  // ---- orbfe_project_sim3 ----
  EXPECT(!sim3_check_legs(cap, 3, off3.data(), slot.data(), legs.data(), 0));
  EXPECT(!sim3_check_legs(cap, 3, off3.data(), slot.data(), legs.data(), 8));
  EXPECT(!sim3_check_legs(cap, 0, nullptr, nullptr, nullptr, 0));  // nothing to do, whatever the pointers
  {
    std::vector<int32_t> off128(129, 0);  // 128 empty legs
    auto l128 = legs_of(128, 8);
    EXPECT(!sim3_check_legs(cap, 128, off128.data(), nullptr, l128.data(), 0));
  }
  // the leg count -- checked before any array of n_legs entries is read (legs holds three, off3 four)
  EXPECT(says(sim3_check_legs(cap, 129, off3.data(), slot.data(), legs.data(), 0), "128 legs"));
  EXPECT(says(sim3_check_legs(cap, -1, off3.data(), slot.data(), legs.data(), 0), "negative number"));
  EXPECT(says(sim3_check_legs(cap, 3, nullptr, slot.data(), legs.data(), 0), "NULL offsets"));
  {
    std::vector<int32_t> o = {1, 4, 4, 6};
    EXPECT(says(sim3_check_legs(cap, 3, o.data(), slot.data(), legs.data(), 0), "start at 0"));
    o = {0, 4, 3, 6};
    EXPECT(says(sim3_check_legs(cap, 3, o.data(), slot.data(), legs.data(), 0), "descend"));
    o = {0, 4, 6, 5};  // (the last step: a check that stops early would miss it)
    EXPECT(says(sim3_check_legs(cap, 3, o.data(), slot.data(), legs.data(), 0), "descend"));
    const int32_t neg[2] = {0, -1};
    EXPECT(says(sim3_check_legs(cap, 1, neg, slot.data(), legs.data(), 0), "negative count"));
  }
  // slots: -1 is "no map point" here; anything below, or at or past the capacity, is refused
  EXPECT(says(sim3_check_legs(cap, 3, off3.data(), nullptr, legs.data(), 0), "NULL slot list"));
  for (int32_t bad : {100, -2, 1 << 30}) {
    std::vector<int32_t> s = slot;
    s[5] = bad;  // (the last entry)
    EXPECT(says(sim3_check_legs(cap, 3, off3.data(), s.data(), legs.data(), 0), "slot outside"));
  }
  EXPECT(says(sim3_check_legs(cap, 3, off3.data(), slot.data(), nullptr, 0), "NULL leg"));
  {
    auto l = legs;
    l[2].n_levels = 9;
    EXPECT(says(sim3_check_legs(cap, 3, off3.data(), slot.data(), l.data(), 8), "more levels"));
    EXPECT(!sim3_check_legs(cap, 3, off3.data(), slot.data(), l.data(), 0));
    l[2].n_levels = 0;
    EXPECT(says(sim3_check_legs(cap, 3, off3.data(), slot.data(), l.data(), 0), "n_levels must be"));
    l[2].n_levels = 65;
    EXPECT(says(sim3_check_legs(cap, 3, off3.data(), slot.data(), l.data(), 0), "n_levels must be"));
  }

  // ---- orbfe_search_by_sim3_mappoints_multi: n1 = 3 keypoints in KF1, K = 2 candidates of 2 and 1 keypoints ----
  const int n1 = 3, K = 2;
  std::vector<int32_t> slot1 = {7, -1, 99}, off2 = {0, 2, 3}, slot2 = {1, -1, 2}, matched = {-1, 5, -1, 99, -1, -1}, kf = {0, 15};
  auto l12 = legs_of(K, 8), l21 = legs_of(K, 8);
  auto check = [&](int k, const int32_t* s1, const int32_t* o2, const int32_t* s2, const orbfe_sim3_leg* a, const orbfe_sim3_leg* b,
                   const int32_t* m, const int32_t* kfs, bool graph, int levels) {
    return sim3_check_search(cap, n1, s1, k, o2, s2, a, b, m, kfs, graph, 16, levels);
  };
  EXPECT(!check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), matched.data(), kf.data(), true, 8));
  EXPECT(!check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8));
  EXPECT(!check(0, slot1.data(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, false, 8));
  EXPECT(says(check(65, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "64 candidates"));
  EXPECT(says(check(-1, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "negative number"));
  for (int levels : {0, 65, -3})
    EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, levels), "n_levels must be"));
  EXPECT(says(check(K, nullptr, off2.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "NULL slot list"));
  EXPECT(says(check(K, slot1.data(), nullptr, slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "NULL offsets"));
  EXPECT(says(check(K, slot1.data(), off2.data(), nullptr, l12.data(), l21.data(), nullptr, nullptr, false, 8), "NULL slot list"));
  EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), nullptr, l21.data(), nullptr, nullptr, false, 8), "NULL leg"));
  EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), nullptr, nullptr, nullptr, false, 8), "NULL leg"));
  {
    std::vector<int32_t> s = slot1;
    s[2] = 100;
    EXPECT(says(check(K, s.data(), off2.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "slot outside"));
    s = slot2;
    s[2] = -2;
    EXPECT(says(check(K, slot1.data(), off2.data(), s.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "slot outside"));
    std::vector<int32_t> o = {0, 2, 1};
    EXPECT(says(check(K, slot1.data(), o.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "descend"));
    o = {2, 2, 3};
    EXPECT(says(check(K, slot1.data(), o.data(), slot2.data(), l12.data(), l21.data(), nullptr, nullptr, false, 8), "start at 0"));
    std::vector<int32_t> m = matched;
    m[5] = 100;  // (the last entry of K * n1)
    EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), m.data(), nullptr, false, 8), "matched slot"));
    m[5] = -2;
    EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), m.data(), nullptr, false, 8), "matched slot"));
    auto l = l21;
    l[1].n_levels = 9;
    EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l.data(), nullptr, nullptr, false, 8), "more levels"));
  }
  EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), matched.data(), nullptr, true, 8), "NULL kf2_slot"));
  for (int32_t bad : {16, -1}) {
    std::vector<int32_t> k2 = kf;
    k2[1] = bad;
    EXPECT(says(check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), matched.data(), k2.data(), true, 8), "kf slot outside"));
    EXPECT(!check(K, slot1.data(), off2.data(), slot2.data(), l12.data(), l21.data(), matched.data(), k2.data(), false, 8));
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
