// The host checks of the key-frame descriptor store and of the distinctive-descriptor loop (csrc/obsgraph_host.h:
// enable_keyframe_descriptors, check_set_keyframe_descriptors, check_distinctive, clear) and the flat restatement next to
// them, as a stand-alone program for -fsanitize=address,undefined: every array is a heap block exactly as long as the
// call says, so a read or write past it is reported.  The winners are worked out by hand from src/MapPoint.cc:288-328 on
// descriptors whose first v bits are set (distance |v - w|).  Prints "ok".
#include <cstdio>
#include <cstdlib>
#include <cstring>
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

static void bits(uint8_t* d, int v) {
  std::memset(d, 0, 32);
  for (int b = 0; b < v; b++) d[b / 8] |= (uint8_t)(0x80 >> (b % 8));
}

int main() {
  const int P = 10, K = 6, W = 64;
  ObsGraphMirror g;
  g.init(P, K, 8);
  {  // not enabled: everything refuses, nothing is allocated
    I32 s = {1};
    CHECK(g.check_set_keyframe_descriptors(0, 1, true) && g.check_distinctive(1, s.data()) && g.descN.empty());
    g.clear();
    CHECK(g.descN.empty() && g.kfDescWidth == 0);
  }
  CHECK(g.enable_keyframe_descriptors(0) && g.enable_keyframe_descriptors(100) && g.enable_keyframe_descriptors(32) &&
        g.enable_keyframe_descriptors(16448) && g.enable_keyframe_descriptors(-64));
  CHECK(!g.enable_keyframe_descriptors(W) && !g.enable_keyframe_descriptors(W) && g.enable_keyframe_descriptors(128) && g.kfDescWidth == W);
  CHECK(g.descN.size() == (size_t)K && g.kfRows.empty());  // independent of the key-frame rows
  {
    ObsGraphMirror big;
    big.init(8, (1 << 12) + 1, 8);
    CHECK(big.enable_keyframe_descriptors(16384) && !big.enable_keyframe_descriptors(8192));
  }
  {
    I32 kf = {0, 1, 2, 3, 4};  // kf slot 5 is never set
    std::vector<int64_t> id = {50, 40, 30, 20, 10};
    std::vector<float> ow(15, 0.f);
    std::vector<uint8_t> bad = {0, 0, 0, 1, 0};  // kf slot 3 is bad
    CHECK(!g.set_keyframes(5, kf.data(), id.data(), ow.data(), bad.data()));
    I32 slot = {0, 1, 2, 3, 4, 5, 6, 7};  // point slots 8, 9 are never set: they count as bad
    I32 ref(8, 0);
    std::vector<uint8_t> pbad = {0, 0, 0, 0, 0, 0, 1, 0};  // 6 is bad
    CHECK(!g.set_points(8, slot.data(), pbad.data(), ref.data()));
  }
  // set: kf slot, count, source
  CHECK(!g.check_set_keyframe_descriptors(0, 0, false) && !g.check_set_keyframe_descriptors(0, W, true));
  CHECK(g.check_set_keyframe_descriptors(0, W + 1, true) && g.check_set_keyframe_descriptors(0, -1, true) && g.check_set_keyframe_descriptors(0, 1, false));
  CHECK(g.check_set_keyframe_descriptors(5, 1, true) && g.check_set_keyframe_descriptors(K, 1, true) && g.check_set_keyframe_descriptors(-1, 1, true));
  {  // rows: 0 = kf 4, 2, 1, 0 (ascending id) at idx 0, 1, 2, 3;  1 = kf 3 (bad) and kf 0;  6 = a bad point with an entry;  7 empty
    I32 slot = {0, 0, 0, 0, 1, 1, 6}, kf = {0, 1, 2, 4, 3, 0, 2};
    std::vector<uint16_t> idx = {3, 2, 1, 0, 5, 4, 63};
    std::vector<uint8_t> oct(7, 0), st(7, 0);
    bool full;
    CHECK(!g.add_observations(7, slot.data(), kf.data(), idx.data(), oct.data(), st.data(), &full));
    g.meta[6].bad = 1;
  }
  I32 all = {0, 1, 6, 7, 9}, one = {1}, out = {0, P}, low = {-1};
  CHECK(g.check_distinctive(5, all.data()));  // nothing was set
  g.descN = {5, 3, 2, 6, 1, 0};
  CHECK(!g.check_distinctive(5, all.data()) && !g.check_distinctive(0, nullptr));
  CHECK(g.check_distinctive(2, out.data()) && g.check_distinctive(1, low.data()));
  g.descN[3] = 5;  // idx 5 of the BAD key frame 3 is not below its count: refused all the same
  CHECK(g.check_distinctive(1, one.data()) && g.check_distinctive(5, all.data()));
  g.descN[3] = 0;
  CHECK(g.check_distinctive(1, one.data()));
  g.descN[3] = 6;
  g.descN[2] = 1;  // the bad point 6 names idx 63 of kf 2, and row 0 names idx 1: only the latter counts
  I32 six = {6};
  CHECK(!g.check_distinctive(1, six.data()) && g.check_distinctive(5, all.data()));
  g.descN[2] = 2;
  CHECK(!g.check_distinctive(5, all.data()));

  // the flat restatement on the arrays the device holds, each exactly as large as it is
  std::vector<uint8_t> desc((size_t)K * W * 32, 0xff);
  auto put = [&](int kf, int idx, int v) { bits(desc.data() + ((size_t)kf * W + idx) * 32, v); };
  // row 0 in table order: kf 4 idx 0, kf 2 idx 1, kf 1 idx 2, kf 0 idx 3 -> values 0, 8, 9, 20: k = 1, medians 8, 1, 1, 11
  put(4, 0, 0); put(2, 1, 8); put(1, 2, 9); put(0, 3, 20);
  put(3, 5, 77); put(0, 4, 3);
  {
    const std::vector<ObsEntry> r0 = g.rows[0], r1 = g.rows[1];
    CHECK(r0.size() == 4 && r0[0].kf == 4 && r0[3].kf == 0 && r1.size() == 2 && r1[0].kf == 3);
    CHECK(obsdesc_distinctive_flat(r0.data(), 4, g.kfs.data(), desc.data(), W) == 1);
    CHECK(obsdesc_distinctive_flat(r0.data(), 2, g.kfs.data(), desc.data(), W) == 0);  // N = 2: the first
    CHECK(obsdesc_distinctive_flat(r0.data(), 1, g.kfs.data(), desc.data(), W) == 0);
    CHECK(obsdesc_distinctive_flat(r0.data(), 0, g.kfs.data(), desc.data(), W) == -1);
    CHECK(obsdesc_distinctive_flat(r1.data(), 2, g.kfs.data(), desc.data(), W) == 1);  // the bad key frame is skipped
    CHECK(obsdesc_distinctive_flat(r1.data(), 1, g.kfs.data(), desc.data(), W) == -1);  // ... and nothing remains
    g.kfs[2].bad = 1;  // values 0, 9, 20: k = 1, medians 9, 9, 11 -> the first
    CHECK(obsdesc_distinctive_flat(r0.data(), 4, g.kfs.data(), desc.data(), W) == 0);
    g.kfs[4].bad = 1;  // values 9, 20 -> the first that remains: row position 2
    CHECK(obsdesc_distinctive_flat(r0.data(), 4, g.kfs.data(), desc.data(), W) == 2);
  }
  g.clear();  // every count back to 0, the width stays
  CHECK(g.kfDescWidth == W && g.descN == I32((size_t)K, 0) && g.enable_keyframe_descriptors(128) && !g.enable_keyframe_descriptors(W));
  std::printf("ok\n");
  return 0;
}
