// Stand-alone program: the host side of the device map-point table (csrc/mappoints_host.h: argument checks, the slab
// layout, the interleaving of an update's records) on exactly-sized heap buffers, up to where orbfe_mappoints_create / _update /
// _destroy would make their first device call.  Built with -fsanitize=address,undefined and run on the CPU
// (tests/test_mappoints_host_san.py); nothing of it is loaded into Python.  Prints "ok" and returns 0.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "mappoints_host.h"

using namespace orbfe;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

int main() {
  // create
  void* out = nullptr;
  EXPECT(mappoints_check_create(4096, &out) == nullptr);
  EXPECT(mappoints_check_create(0, &out) && mappoints_check_create(-5, &out) && mappoints_check_create(kMapPointsMaxCapacity + 1, &out));
  EXPECT(mappoints_check_create(16, nullptr));
  for (int cap : {1, 7, 255, 256, 257, 4096, kMapPointsMaxCapacity}) {
    const MapPointsLayout L = mappoints_layout(cap);
    EXPECT(L.oRec == 0 && L.oDesc >= (size_t)cap * 32 && L.oFlags >= L.oDesc + (size_t)cap * 32 && L.total >= L.oFlags + (size_t)cap);
    EXPECT(L.oDesc % 256 == 0 && L.oFlags % 256 == 0 && L.total % 256 == 0);
  }
  // update: every n around the alignment steps, every array exactly n entries long (slots, flags and descriptors travel as
  // they are, through the arena's own up(): the records are what this file packs)
  const int cap = 300;
  for (int n : {0, 1, 2, 63, 64, 65, 255, 256, 257, 300}) {
    auto slot = exact<int32_t>(n);
    auto pos = exact<float>(3 * (size_t)n), normal = exact<float>(3 * (size_t)n), lo = exact<float>(n), hi = exact<float>(n);
    auto flags = exact<uint8_t>(n);
    for (int i = 0; i < n; i++) {
      slot[i] = (i * 7 + 3) % cap;
      for (int k = 0; k < 3; k++) { pos[3 * i + k] = (float)(i + k); normal[3 * i + k] = (float)(k - i); }
      lo[i] = 0.5f * i; hi[i] = 2.0f * i; flags[i] = (uint8_t)(i & 3);
    }
    EXPECT(mappoints_check_update(cap, n, slot.get(), pos.get(), normal.get(), lo.get(), hi.get(), flags.get()) == nullptr);
    auto rec = exact<float>(8 * (size_t)n);
    mappoints_pack_records(rec.get(), n, pos.get(), normal.get(), lo.get(), hi.get());
    for (int i = 0; i < n; i++) {
      const float* r = rec.get() + 8 * (size_t)i;
      EXPECT(r[0] == pos[3 * i] && r[1] == pos[3 * i + 1] && r[2] == pos[3 * i + 2] && r[3] == lo[i]);
      EXPECT(r[4] == normal[3 * i] && r[5] == normal[3 * i + 1] && r[6] == normal[3 * i + 2] && r[7] == hi[i]);
    }
    // refused before anything is staged: slots outside the table, NULL arrays, a negative count
    if (n > 0) {
      for (int32_t bad : {-1, cap, INT32_MAX, INT32_MIN}) {
        const int32_t keep = slot[n - 1];
        slot[n - 1] = bad;
        EXPECT(mappoints_check_update(cap, n, slot.get(), pos.get(), normal.get(), lo.get(), hi.get(), flags.get()) != nullptr);
        EXPECT(mappoints_check_slots(cap, n, slot.get()) != nullptr);
        slot[n - 1] = keep;
      }
      EXPECT(mappoints_check_update(cap, n, nullptr, pos.get(), normal.get(), lo.get(), hi.get(), flags.get()) != nullptr);
      EXPECT(mappoints_check_update(cap, n, slot.get(), nullptr, normal.get(), lo.get(), hi.get(), flags.get()) != nullptr);
      EXPECT(mappoints_check_update(cap, n, slot.get(), pos.get(), nullptr, lo.get(), hi.get(), flags.get()) != nullptr);
      EXPECT(mappoints_check_update(cap, n, slot.get(), pos.get(), normal.get(), nullptr, hi.get(), flags.get()) != nullptr);
      EXPECT(mappoints_check_update(cap, n, slot.get(), pos.get(), normal.get(), lo.get(), nullptr, flags.get()) != nullptr);
      EXPECT(mappoints_check_update(cap, n, slot.get(), pos.get(), normal.get(), lo.get(), hi.get(), nullptr) != nullptr);
    }
    EXPECT(mappoints_check_update(cap, -1, slot.get(), pos.get(), normal.get(), lo.get(), hi.get(), flags.get()) != nullptr);
  }
  EXPECT(mappoints_check_update(cap, 0, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr) == nullptr);
  std::printf("ok\n");
  return 0;
}
