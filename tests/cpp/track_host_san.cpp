// The argument checks of orbfe_project_last_frame / orbfe_search_last_frame_mappoints / orbfe_project_keyframe /
// orbfe_search_keyframe_mappoints_multi that need no device (csrc/mappoints_host.h: track_check_operands) as a stand-alone
// program, built with the address and undefined-behaviour sanitizers by tests/test_track_host.py: every array is exactly as
// long as the call says, so a check that reads past one is reported.
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
  const int cap = 100;
  std::vector<int32_t> slot = {0, 99, 5, 5, 42, 7};
  std::vector<int32_t> oct = {0, 7, 3, 3, 1, 2};
  std::vector<int32_t> off3 = {0, 4, 4, 6};  // three jobs, the middle one empty
  std::vector<int32_t> off1 = {0, 6};
  std::vector<orbfe_camera_pose> pose(64);
  for (auto& p : pose) { std::memset(&p, 0, sizeof p); p.n_levels = 8; }

  // good calls: the last-frame form (K = 1, octaves), the key-frame form (K jobs, no octaves), with and without a level table
  EXPECT(!track_check_operands(cap, 1, off1.data(), slot.data(), true, oct.data(), pose.data(), 8));
  EXPECT(!track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, pose.data(), 8));
  EXPECT(!track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, pose.data(), 0));
  {
    std::vector<int32_t> off64(65, 0);  // 64 empty jobs
    EXPECT(!track_check_operands(cap, 64, off64.data(), nullptr, false, nullptr, pose.data(), 8));
  }
  // nothing to do is fine, whatever the pointers
  EXPECT(!track_check_operands(cap, 0, nullptr, nullptr, false, nullptr, nullptr, 8));
  {
    const int32_t none[2] = {0, 0};
    EXPECT(!track_check_operands(cap, 1, none, nullptr, true, nullptr, pose.data(), 8));
  }

  // K bounds -- checked before any array of K entries is read (pose holds 64, off3 four)
  EXPECT(says(track_check_operands(cap, 65, off3.data(), slot.data(), false, nullptr, pose.data(), 8), "64 jobs"));
  EXPECT(says(track_check_operands(cap, -1, off3.data(), slot.data(), false, nullptr, pose.data(), 8), "negative number"));
  // offsets
  EXPECT(says(track_check_operands(cap, 3, nullptr, slot.data(), false, nullptr, pose.data(), 8), "NULL offsets"));
  {
    std::vector<int32_t> o = {1, 4, 4, 6};
    EXPECT(says(track_check_operands(cap, 3, o.data(), slot.data(), false, nullptr, pose.data(), 8), "start at 0"));
    o = {0, 4, 3, 6};
    EXPECT(says(track_check_operands(cap, 3, o.data(), slot.data(), false, nullptr, pose.data(), 8), "descend"));
    o = {0, 4, 6, 5};  // (the last step: a check that stops early would miss it)
    EXPECT(says(track_check_operands(cap, 3, o.data(), slot.data(), false, nullptr, pose.data(), 8), "descend"));
    const int32_t neg[2] = {0, -1};
    EXPECT(says(track_check_operands(cap, 1, neg, slot.data(), true, oct.data(), pose.data(), 8), "negative count"));
  }
  // slots: -1 stays invalid, as everywhere else on this table
  EXPECT(says(track_check_operands(cap, 1, off1.data(), nullptr, true, oct.data(), pose.data(), 8), "NULL slot list"));
  for (int32_t bad : {100, -1, 1 << 30}) {
    std::vector<int32_t> s = slot;
    s[5] = bad;  // (the last entry)
    EXPECT(says(track_check_operands(cap, 1, off1.data(), s.data(), true, oct.data(), pose.data(), 8), "slot outside"));
    EXPECT(says(track_check_operands(cap, 3, off3.data(), s.data(), false, nullptr, pose.data(), 8), "slot outside"));
  }
  // octaves inside the level table, read only by the last-frame form
  EXPECT(says(track_check_operands(cap, 1, off1.data(), slot.data(), true, nullptr, pose.data(), 8), "NULL octave"));
  for (int32_t bad : {8, -1}) {
    std::vector<int32_t> o = oct;
    o[5] = bad;
    EXPECT(says(track_check_operands(cap, 1, off1.data(), slot.data(), true, o.data(), pose.data(), 8), "octave outside"));
    EXPECT(!track_check_operands(cap, 1, off1.data(), slot.data(), false, o.data(), pose.data(), 8));
  }
  // the poses
  EXPECT(says(track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, nullptr, 8), "NULL pose"));
  {
    std::vector<orbfe_camera_pose> p(pose.begin(), pose.begin() + 3);
    p[2].n_levels = 9;
    EXPECT(says(track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, p.data(), 8), "more levels"));
    EXPECT(!track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, p.data(), 0));  // (orbfe_project_keyframe has no table)
    p[2].n_levels = 0;
    EXPECT(says(track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, p.data(), 8), "n_levels must be"));
    p[2].n_levels = 65;
    EXPECT(says(track_check_operands(cap, 3, off3.data(), slot.data(), false, nullptr, p.data(), 0), "n_levels must be"));
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
