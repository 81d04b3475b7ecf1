// The argument checks of orbfe_project_fuse / orbfe_fuse_mappoints that need no device (csrc/mappoints_host.h:
// fuse_check_operands) as a stand-alone program, built with the address and undefined-behaviour sanitizers by
// tests/test_fuse_host.py: every array is exactly as long as the call says, so a check that reads past one is reported.
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

int main() {
  const int cap = 100, kfCap = 16;
  std::vector<int32_t> slot = {0, 99, 5, 5, 42};
  const int n = (int)slot.size();
  std::vector<orbfe_camera_pose> pose(64);
  for (auto& p : pose) { std::memset(&p, 0, sizeof p); p.n_levels = 8; }
  std::vector<int32_t> kf = {0, 15, 3};

  // good calls, with and without a graph, with and without level tables
  EXPECT(!fuse_check_operands(cap, n, slot.data(), 3, kf.data(), true, kfCap, pose.data(), 8));
  EXPECT(!fuse_check_operands(cap, n, slot.data(), 3, nullptr, false, 0, pose.data(), 0));
  EXPECT(!fuse_check_operands(cap, n, slot.data(), 64, nullptr, false, 0, pose.data(), 8));
  // nothing to do is fine, whatever the pointers
  EXPECT(!fuse_check_operands(cap, 0, nullptr, 3, kf.data(), true, kfCap, pose.data(), 8));
  EXPECT(!fuse_check_operands(cap, n, slot.data(), 0, nullptr, true, kfCap, nullptr, 8));
  EXPECT(!fuse_check_operands(cap, 0, nullptr, 0, nullptr, false, 0, nullptr, 0));

  // K: at most 64 -- checked before any array of K entries is read (pose holds 64)
  EXPECT(says(fuse_check_operands(cap, n, slot.data(), 65, nullptr, false, 0, pose.data(), 8), "64 key frames"));
  EXPECT(says(fuse_check_operands(cap, n, slot.data(), -1, nullptr, false, 0, pose.data(), 8), "negative"));
  // slots
  EXPECT(says(fuse_check_operands(cap, -1, slot.data(), 3, nullptr, false, 0, pose.data(), 8), "negative count"));
  EXPECT(says(fuse_check_operands(cap, n, nullptr, 3, nullptr, false, 0, pose.data(), 8), "NULL slot list"));
  for (int32_t bad : {100, -1, 1 << 30}) {
    std::vector<int32_t> s = slot;
    s[4] = bad;  // (the last entry: a check that stops early would miss it)
    EXPECT(says(fuse_check_operands(cap, n, s.data(), 3, nullptr, false, 0, pose.data(), 8), "slot outside"));
  }
  // NULL arrays
  EXPECT(says(fuse_check_operands(cap, n, slot.data(), 3, nullptr, false, 0, nullptr, 8), "NULL pose"));
  EXPECT(says(fuse_check_operands(cap, n, slot.data(), 3, nullptr, true, kfCap, pose.data(), 8), "NULL kf_slot"));
  // kf slots are read only with a graph
  for (int32_t bad : {16, -1}) {
    std::vector<int32_t> k = kf;
    k[2] = bad;
    EXPECT(says(fuse_check_operands(cap, n, slot.data(), 3, k.data(), true, kfCap, pose.data(), 8), "kf slot outside"));
    EXPECT(!fuse_check_operands(cap, n, slot.data(), 3, k.data(), false, kfCap, pose.data(), 8));
  }
  // the poses' level counts
  {
    std::vector<orbfe_camera_pose> p(pose.begin(), pose.begin() + 3);
    p[2].n_levels = 9;
    EXPECT(says(fuse_check_operands(cap, n, slot.data(), 3, nullptr, false, 0, p.data(), 8), "more levels"));
    EXPECT(!fuse_check_operands(cap, n, slot.data(), 3, nullptr, false, 0, p.data(), 0));  // (orbfe_project_fuse has no tables)
    p[2].n_levels = 0;
    EXPECT(says(fuse_check_operands(cap, n, slot.data(), 3, nullptr, false, 0, p.data(), 8), "n_levels must be"));
    p[2].n_levels = 65;
    EXPECT(says(fuse_check_operands(cap, n, slot.data(), 3, nullptr, false, 0, p.data(), 0), "n_levels must be"));
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
