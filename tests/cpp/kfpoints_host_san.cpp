// The key-frame rows of the observation graph's host mirror (csrc/obsgraph_host.h: enable / set / assign / clear, the
// query checks) and the flat ordered union and TrackedMapPoints next to them, as a stand-alone program for
// -fsanitize=address,undefined: every array is a heap block exactly as long as the call says, so a read or write past it
// is reported.  The union's answers are worked out by hand from src/Tracking.cc:1315-1333.  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "obsgraph_host.h"

using namespace orbfe;

#define CHECK(c)                                            \
  do {                                                      \
    if (!(c)) {                                             \
      std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); \
      return 1;                                             \
    }                                                       \
  } while (0)

typedef std::vector<int32_t> I32;

int main() {
  const int P = 12, K = 6, W = 64;
  ObsGraphMirror g;
  g.init(P, K, 8);
  {  // not enabled: everything refuses, nothing is allocated
    I32 s = {1};
    std::vector<uint16_t> i0 = {0};
    CHECK(g.set_keyframe_points(0, 1, s.data()) && g.assign_keyframe_points(1, s.data(), i0.data(), s.data()));
    CHECK(g.check_kf_list(1, s.data()) && g.kfRows.empty() && g.kfRowDirty.empty());
    g.clear();
    CHECK(g.kfRows.empty());
  }
  CHECK(g.enable_keyframe_points(0) && g.enable_keyframe_points(96 + 4) && g.enable_keyframe_points(32) && g.enable_keyframe_points(16448));
  CHECK(!g.enable_keyframe_points(W) && !g.enable_keyframe_points(W) && g.enable_keyframe_points(128) && g.kfRowWidth == W);
  {
    I32 kf = {0, 1, 2, 3, 4};  // kf slot 5 is never set
    std::vector<int64_t> id = {50, 40, 30, 20, 10};
    std::vector<float> ow(15, 0.f);
    std::vector<uint8_t> bad(5, 0);
    CHECK(!g.set_keyframes(5, kf.data(), id.data(), ow.data(), bad.data()));
    I32 slot = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9};  // point slots 10, 11 are never set: they count as bad
    I32 ref(10, 0);
    std::vector<uint8_t> pbad = {0, 0, 0, 0, 0, 0, 0, 0, 1, 0};  // 8 is bad
    CHECK(!g.set_points(10, slot.data(), pbad.data(), ref.data()));
  }
  g.dirtyKfRows.clear();
  {
    I32 r0 = {5, -1, 7, 5, 9}, r1 = {7, 3, -1, 8, 11}, r3 = {8, 2, 3, -1, 5}, full((size_t)W, -1), over((size_t)W + 1, -1);
    I32 wrong = {5, 12}, low = {-2};
    CHECK(!g.set_keyframe_points(0, 5, r0.data()) && !g.set_keyframe_points(1, 5, r1.data()) && !g.set_keyframe_points(3, 5, r3.data()));
    CHECK(!g.set_keyframe_points(2, 0, nullptr) && !g.set_keyframe_points(4, W, full.data()));
    CHECK(g.set_keyframe_points(4, W + 1, over.data()) && g.set_keyframe_points(5, 5, r0.data()) && g.set_keyframe_points(6, 5, r0.data()));
    CHECK(g.set_keyframe_points(0, 2, wrong.data()) && g.set_keyframe_points(0, 1, low.data()) && g.set_keyframe_points(0, -1, r0.data()));
    CHECK(g.set_keyframe_points(0, 2, nullptr));
    CHECK(g.kfRows[0] == r0 && g.kfRows[4].size() == (size_t)W && g.dirtyKfRows.size() == 5);
  }
  {  // assign: as a whole or not at all
    I32 kf = {0, 1, 0}, slot = {4, -1, 6};
    std::vector<uint16_t> idx = {1, 0, 5};  // idx 5 is the length of row 0
    CHECK(g.assign_keyframe_points(3, kf.data(), idx.data(), slot.data()));
    CHECK(g.kfRows[0][1] == -1 && g.kfRows[1][0] == 7);
    idx[2] = 4;
    slot[2] = P;
    CHECK(g.assign_keyframe_points(3, kf.data(), idx.data(), slot.data()) && g.kfRows[0][1] == -1);
    slot[2] = 6;
    kf[1] = K;
    CHECK(g.assign_keyframe_points(3, kf.data(), idx.data(), slot.data()) && g.kfRows[0][1] == -1);
    kf[1] = 1;
    CHECK(!g.assign_keyframe_points(3, kf.data(), idx.data(), slot.data()));
    CHECK((g.kfRows[0] == I32{5, 4, 7, 5, 6}) && (g.kfRows[1] == I32{-1, 3, -1, 8, 11}));
    std::vector<uint16_t> i2 = {1, 0, 4};
    I32 back = {-1, 7, 9};
    CHECK(!g.assign_keyframe_points(3, kf.data(), i2.data(), back.data()));
    CHECK(!g.assign_keyframe_points(0, nullptr, nullptr, nullptr) && g.assign_keyframe_points(1, kf.data(), nullptr, back.data()));
  }
  {  // the query checks
    I32 off = {0, 2, 2, 5}, kfs = {0, 1, 3, 2, 3}, desc = {0, 2, 1, 5}, late = {1, 2, 2, 5}, unset = {0, 5, 3, 2, 3}, out = {0, K, 3, 2, 3};
    CHECK(!g.check_kf_queries(3, off.data(), kfs.data()));
    CHECK(g.check_kf_queries(3, desc.data(), kfs.data()) && g.check_kf_queries(3, late.data(), kfs.data()));
    CHECK(g.check_kf_queries(3, off.data(), unset.data()) && g.check_kf_queries(3, off.data(), out.data()) && g.check_kf_queries(3, off.data(), nullptr));
    I32 none = {0, 0};
    CHECK(!g.check_kf_queries(1, none.data(), nullptr));
  }
  // the flat arrays the device holds, each exactly as large as it is
  I32 rows((size_t)K * W, -1), len((size_t)K, 0);
  for (int k = 0; k < K; k++) {
    len[(size_t)k] = (int32_t)g.kfRows[(size_t)k].size();
    for (size_t i = 0; i < g.kfRows[(size_t)k].size(); i++) rows[(size_t)k * W + i] = g.kfRows[(size_t)k][i];
  }
  std::vector<ObsPointMeta> meta = g.meta;
  I32 stamp((size_t)P, 0);
  int32_t mark = 0;
  struct Case { I32 kfs, want; };
  // rows: 0 = [5 NULL 7 5 9], 1 = [7 3 NULL 8 11], 2 = [], 3 = [8 2 3 NULL 5], 4 = 64 x NULL; 8 is bad, 11 was never set
  const std::vector<Case> cases = {
      {{0}, {5, 7, 9}},            {{0, 1}, {5, 7, 9, 3}},       {{1, 0}, {7, 3, 5, 9}}, {{3, 2, 1, 0}, {2, 3, 5, 7, 9}},
      {{1, 1}, {7, 3}},            {{0, 1, 0, 3, 1}, {5, 7, 9, 3, 2}}, {{2}, {}},        {{4, 2}, {}},
      {{}, {}},
  };
  for (const Case& c : cases) {
    I32 got(c.want.size(), -7);  // capacity exactly the count
    const int n = kfpoints_union_flat(rows.data(), len.data(), W, meta.data(), (int)c.kfs.size(), c.kfs.data(), stamp.data(), ++mark, got.data(),
                                      (int)got.size());
    CHECK(n == (int)c.want.size() && got == c.want);
    if (!c.want.empty()) {  // one short: the count stands, the prefix is written, nothing past it
      I32 few(c.want.size() - 1, -7);
      const int m = kfpoints_union_flat(rows.data(), len.data(), W, meta.data(), (int)c.kfs.size(), c.kfs.data(), stamp.data(), ++mark, few.data(),
                                        (int)few.size());
      CHECK(m == n && few == I32(c.want.begin(), c.want.end() - 1));
    }
  }
  {  // TrackedMapPoints: nObs 5 -> 4, 7 -> 1, 9 -> 2, 3 -> 3, 2 -> 0; bad 8 holds 9
    const int nobs[10] = {0, 0, 0, 3, 0, 4, 0, 1, 9, 2};
    for (int s = 0; s < 10; s++) meta[(size_t)s].nObs = nobs[s];
    const int want0[4] = {4, 4, 3, 2}, want3[4] = {3, 2, 2, 2}, mins[4] = {0, 1, 2, 3};
    for (int i = 0; i < 4; i++) {
      CHECK(kfpoints_tracked_flat(rows.data(), len[0], meta.data(), mins[i]) == want0[i]);
      CHECK(kfpoints_tracked_flat(rows.data() + 3 * W, len[3], meta.data(), mins[i]) == want3[i]);
    }
    CHECK(kfpoints_tracked_flat(rows.data() + 2 * W, len[2], meta.data(), 0) == 0);
    CHECK(kfpoints_tracked_flat(rows.data() + 4 * W, len[4], meta.data(), 0) == 0);
  }
  g.clear();  // empties the rows, keeps the width, marks every row
  CHECK(g.kfRowWidth == W && g.kfRows[0].empty() && g.kfRows[4].empty() && g.dirtyKfRows.size() == (size_t)K);
  g.kf_rows_flushed();
  CHECK(g.dirtyKfRows.empty());
  std::printf("ok\n");
  return 0;
}
