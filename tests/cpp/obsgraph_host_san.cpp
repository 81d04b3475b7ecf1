// The host side of the device observation graph (csrc/obsgraph_host.h: the mirror, the argument checks and the two
// replays) as a stand-alone program for -fsanitize=address,undefined: every array is a heap block exactly as long as the
// call says, so a read or write past it is reported.  Prints "ok".
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

int main() {
  int dummy;
  CHECK(!obsgraph_check_create(0, 16, 8, 8, &dummy));
  CHECK(obsgraph_check_create(0, 16, 8, 12, &dummy) && obsgraph_check_create(0, 0, 8, 8, &dummy) && obsgraph_check_create(0, 16, 8, 8, nullptr));
  ObsGraphMirror g;
  g.init(16, 8, 8);
  {
    std::vector<int32_t> kf = {0, 1, 2, 3, 4, 5, 6, 7};
    std::vector<int64_t> id = {80, 70, 60, 50, 40, 30, 20, 10};
    std::vector<float> ow(24, 0.5f);
    std::vector<uint8_t> bad(8, 0);
    CHECK(!g.set_keyframes(8, kf.data(), id.data(), ow.data(), bad.data()));
    std::vector<int32_t> one = {3};
    std::vector<int64_t> dup = {80};
    CHECK(g.set_keyframes(1, one.data(), dup.data(), ow.data(), bad.data()));  // slot 0 holds id 80
    std::vector<int32_t> out = {8};
    CHECK(g.set_keyframes(1, out.data(), dup.data(), ow.data(), bad.data()));
  }
  {
    std::vector<int32_t> slot(16), ref(16, 0);
    std::vector<uint8_t> bad(16, 0);
    for (int i = 0; i < 16; i++) slot[(size_t)i] = i;
    CHECK(!g.set_points(16, slot.data(), bad.data(), ref.data()));
    slot[15] = 16;
    CHECK(g.set_points(16, slot.data(), bad.data(), ref.data()));
  }
  bool full = false;
  {  // a full row of 8, in ascending id whatever the order of arrival
    std::vector<int32_t> slot(8, 2), kf = {3, 0, 7, 1, 6, 2, 5, 4};
    std::vector<uint16_t> idx = {1, 2, 3, 4, 5, 6, 7, 8};
    std::vector<uint8_t> oct = {0, 1, 2, 3, 4, 5, 6, 7}, st = {1, 0, 1, 0, 1, 0, 1, 0};
    CHECK(!g.add_observations(8, slot.data(), kf.data(), idx.data(), oct.data(), st.data(), &full) && !full);
    CHECK(g.meta[2].count == 8 && g.meta[2].nObs == 12);
    for (int i = 0; i < 8; i++) CHECK(g.rows[2][(size_t)i].kf == 7 - i);
    CHECK(!g.add_observations(8, slot.data(), kf.data(), idx.data(), oct.data(), st.data(), &full));  // all present
    CHECK(g.meta[2].nObs == 12);
    std::vector<int32_t> s2 = {3, 2}, k2 = {1, 1};
    // (2, 1) is present: ignored, so nothing is full
    CHECK(!g.add_observations(2, s2.data(), k2.data(), idx.data(), oct.data(), st.data(), &full) && g.meta[3].count == 1);
  }
  {  // a row of 8 cannot take a ninth: shrink one first
    std::vector<int32_t> s = {2}, k = {4};
    std::vector<uint8_t> bb(1);
    CHECK(!g.erase_observations(1, s.data(), k.data(), bb.data()) && bb[0] == 0 && g.meta[2].count == 7);
    ObsGraphMirror h;
    h.init(4, 12, 8);
    std::vector<int32_t> kf(12);
    std::vector<int64_t> id(12);
    std::vector<float> ow(36, 0.f);
    std::vector<uint8_t> bad(12, 0);
    for (int i = 0; i < 12; i++) { kf[(size_t)i] = i; id[(size_t)i] = i; }
    CHECK(!h.set_keyframes(12, kf.data(), id.data(), ow.data(), bad.data()));
    std::vector<int32_t> slot(9, 1);
    std::vector<uint16_t> idx(9, 0);
    std::vector<uint8_t> z(9, 0);
    slot[0] = 0;  // an entry for another row in front: rolled back with the rest
    CHECK(!h.add_observations(8, slot.data(), kf.data(), idx.data(), z.data(), z.data(), &full));  // row 1: 7 entries
    std::vector<int32_t> s3 = {2, 1, 1}, k3 = {0, 10, 11};
    CHECK(h.add_observations(3, s3.data(), k3.data(), idx.data(), z.data(), z.data(), &full) && full);
    CHECK(h.meta[2].count == 0 && h.meta[1].count == 7 && h.kfRefs[0] == 1 && h.kfRefs[10] == 0 && h.kfPoints[0].size() == 1);
  }
  {  // erase_keyframe: a dry count first, then the erases
    std::vector<int32_t> slot = {5, 5, 5}, kf = {0, 1, 2};
    std::vector<uint16_t> idx(3, 0);
    std::vector<uint8_t> z(3, 0);
    CHECK(!g.add_observations(3, slot.data(), kf.data(), idx.data(), z.data(), z.data(), &full));
    int n = -1;
    bool over = false;
    CHECK(g.erase_keyframe(1, nullptr, 0, &n, &over) && over && n == 2 && g.meta[5].count == 3);  // points 3 and 5 would go
    std::vector<int32_t> out(2, -1);
    CHECK(!g.erase_keyframe(1, out.data(), 2, &n, &over) && n == 2 && out[0] == 3 && out[1] == 5);
    CHECK(g.meta[5].bad && g.meta[5].count == 0 && g.rows[5].empty() && g.kfs[1].bad == 1 && g.kfRefs[1] == 0);
    CHECK(g.meta[2].count == 6 && !g.meta[2].bad);
    CHECK(g.erase_keyframe(8, out.data(), 2, &n, &over) && !over);
  }
  {
    std::vector<int32_t> s = {2, 5, 3};
    CHECK(!g.check_levels(3, s.data(), 8));
    g.meta[2].ref = 7;  // octave 2 in the row above
    CHECK(!g.check_levels(3, s.data(), 3) && g.check_levels(3, s.data(), 2));
  }
  g.clear();
  CHECK(g.meta[2].count == 0 && g.meta[2].bad == 1 && g.kfs[0].id == -1 && (int)g.dirtyRows.size() == 16);
  g.flushed();
  CHECK(g.dirtyRows.empty() && g.kfDirtyLo == g.kfDirtyHi);

  {  // update_connections: outputs of exactly n entries
    std::vector<int64_t> id = {7, 3, 9, 4};
    std::vector<int32_t> w = {15, 14, 15, 20};
    std::vector<int64_t> oi(4), ci(4);
    std::vector<int32_t> ow(4), cw(4);
    int no, nc;
    int64_t parent;
    CHECK(!obsgraph_update_connections(4, id.data(), w.data(), 15, oi.data(), ow.data(), &no, ci.data(), cw.data(), &nc, &parent));
    CHECK(no == 3 && oi[0] == 4 && oi[1] == 9 && oi[2] == 7 && nc == 3 && ci[0] == 4 && ci[1] == 7 && ci[2] == 9 && parent == 4);
    std::vector<int32_t> low = {2, 7, 7, 1};
    CHECK(!obsgraph_update_connections(4, id.data(), low.data(), 15, oi.data(), ow.data(), &no, ci.data(), cw.data(), &nc, &parent));
    CHECK(no == 1 && oi[0] == 3 && ow[0] == 7 && nc == 1 && parent == 3);
    std::vector<int32_t> all = {20, 20, 20, 20};
    CHECK(!obsgraph_update_connections(4, id.data(), all.data(), 15, oi.data(), ow.data(), &no, ci.data(), cw.data(), &nc, &parent));
    CHECK(no == 4 && oi[0] == 9 && oi[3] == 3);
    CHECK(!obsgraph_update_connections(0, nullptr, nullptr, 15, nullptr, nullptr, &no, nullptr, nullptr, &nc, &parent) && no == 0 && parent == -1);
    id[1] = 7;
    CHECK(obsgraph_update_connections(4, id.data(), w.data(), 15, oi.data(), ow.data(), &no, ci.data(), cw.data(), &nc, &parent));
  }
  {  // local_keyframes: CSR arrays exactly as long as the offsets say; out of exactly `capacity`
    std::vector<int64_t> id = {3, 1, 2};
    std::vector<int32_t> w = {3, 1, 3};
    std::vector<uint8_t> bad = {0, 0, 0};
    std::vector<int32_t> no = {0, 1, 3, 5}, co = {0, 1, 2, 2};
    std::vector<int64_t> ni = {30, 2, 10, 10, 12}, ci = {31, 11};
    std::vector<uint8_t> nb(5, 0), cb(2, 0);
    std::vector<int64_t> par = {1, 2, 20};
    std::vector<int64_t> out(7);
    int n;
    int64_t ref;
    bool over;
    CHECK(!obsgraph_local_keyframes(3, id.data(), w.data(), bad.data(), no.data(), ni.data(), nb.data(), co.data(), ci.data(), cb.data(),
                                    par.data(), out.data(), 7, &n, &ref, &over));
    const int64_t want[7] = {1, 2, 3, 10, 11, 12, 20};
    CHECK(n == 7 && ref == 2);
    for (int i = 0; i < 7; i++) CHECK(out[(size_t)i] == want[i]);
    std::vector<int64_t> small(6);
    CHECK(obsgraph_local_keyframes(3, id.data(), w.data(), bad.data(), no.data(), ni.data(), nb.data(), co.data(), ci.data(), cb.data(),
                                   par.data(), small.data(), 6, &n, &ref, &over) && over && n == 7);
    CHECK(!obsgraph_local_keyframes(0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0,
                                    &n, &ref, &over) && n == 0 && ref == -1);
    // 81 voted key frames with no neighbours: the walk stops at once
    std::vector<int64_t> ids(81), pars(81, 500);
    std::vector<int32_t> ws(81, 1), off(82, 0);
    std::vector<uint8_t> bads(81, 0);
    for (int i = 0; i < 81; i++) ids[(size_t)i] = i;
    std::vector<int64_t> big(81);
    CHECK(!obsgraph_local_keyframes(81, ids.data(), ws.data(), bads.data(), off.data(), nullptr, nullptr, off.data(), nullptr, nullptr,
                                    pars.data(), big.data(), 81, &n, &ref, &over) && n == 81 && ref == 0);
  }
  std::printf("ok\n");
  return 0;
}
