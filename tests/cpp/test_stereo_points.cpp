// The stereo-point methods of include/orbfe_classes.hpp -- Tracking::SelectStereoPoints, Tracking::CountClosePoints,
// MapPointTable::CreateStereoPoints -- on a frame made by a formula that tests/test_gpu_stereo_points_cpp.py repeats: prints
// what the classes return, one "key=value" token per result (floats as their bit patterns), for the test to compare with
// the Python binding and the restatement.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

template <typename T>
static void print_ints(const char* key, const std::vector<T>& v) {
  std::printf("%s=", key);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%lld", i ? "," : "", (long long)v[i]);
  std::printf("\n");
}
static void print_bits(const char* key, const std::vector<float>& v) {
  std::vector<int64_t> b;
  for (float x : v) { uint32_t u; std::memcpy(&u, &x, 4); b.push_back((int64_t)u); }
  print_ints(key, b);
}

int main() {
  const int N = 150, CAP = 400, KF = 2;
  std::vector<KeyPoint> keys((size_t)N);
  std::vector<uint8_t> desc((size_t)N * 32), occupied((size_t)N), stale((size_t)N), hasPoint((size_t)N), outlier((size_t)N);
  std::vector<float> uRight((size_t)N), depth((size_t)N), scale;
  for (int k = 0; k < 8; k++) scale.push_back(1.0f + 0.25f * (float)k);
  for (int i = 0; i < N; i++) {
    keys[(size_t)i] = KeyPoint{};
    keys[(size_t)i].x = 20.0f + 4.5f * (float)((i * 37) % 150); keys[(size_t)i].y = 15.0f + 2.75f * (float)((i * 53) % 150);
    keys[(size_t)i].octave = i % 8;
    for (int b = 0; b < 32; b++) desc[(size_t)i * 32 + b] = (uint8_t)((i * 131 + b * 17) % 256);
    // 120 close depths in (0.5, 9.5], every tenth keypoint without depth, the rest far; a tie every 11
    depth[(size_t)i] = i % 10 == 9 ? 0.0f : (i % 5 == 4 ? 12.0f + 0.5f * (float)(i % 13) : 0.5f + 0.0625f * (float)((i * 29) % 144));
    if (i % 11 == 0) depth[(size_t)i] = 4.0f;
    occupied[(size_t)i] = i % 4 == 1;
    stale[(size_t)i] = i % 6 == 2 && !occupied[(size_t)i];
    uRight[(size_t)i] = depth[(size_t)i] > 0 ? (i % 7 == 3 ? -2.0f : keys[(size_t)i].x - 40.0f / depth[(size_t)i]) : -1.0f;
    hasPoint[(size_t)i] = occupied[(size_t)i] || stale[(size_t)i];
    outlier[(size_t)i] = i % 9 == 1;
  }
  FrameArrays F(keys, desc, 0.f, 752.f, 0.f, 480.f, uRight);
  F.makeResident();
  orbfe_camera_pose pose{};
  const float R[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};  // a quarter turn about z
  for (int k = 0; k < 9; k++) pose.Rcw[k] = R[k];
  pose.Ow[0] = 1.5f; pose.Ow[1] = -0.25f; pose.Ow[2] = 0.75f;
  for (int r = 0; r < 3; r++) pose.tcw[r] = -(R[3 * r] * pose.Ow[0] + R[3 * r + 1] * pose.Ow[1] + R[3 * r + 2] * pose.Ow[2]);
  pose.fx = 458.654f; pose.fy = 457.296f; pose.cx = 367.215f; pose.cy = 248.375f; pose.mbf = 40.0f;
  pose.min_x = 0.f; pose.max_x = 752.f; pose.min_y = 0.f; pose.max_y = 480.f;
  pose.log_scale_factor = 0.25f; pose.n_levels = 8;
  const float centre[3] = {1.53125f, -0.3125f, 0.765625f};

  const auto close = Tracking::CountClosePoints(depth, hasPoint, outlier, 10.0f);
  std::printf("tracked_close=%d\nnon_tracked_close=%d\n", close.first, close.second);
  const Tracking::StereoSelection sel = Tracking::SelectStereoPoints(F.x, F.y, F.octave, depth, pose, 10.0f, ORBFE_STEREO_KEYFRAME, scale, centre,
                                                                     occupied, stale);
  print_ints("sel_idx", sel.idx); print_bits("sel_pos", sel.pos); print_bits("sel_normal", sel.normal);
  print_bits("sel_min", sel.minDist); print_bits("sel_max", sel.maxDist); print_ints("sel_cleared", sel.cleared);
  std::printf("sel_walked=%d\n", sel.walked);

  ObservationGraph g(CAP, 4, 8);
  MapPointTable mp(CAP);
  g.SetKeyFrames({0, KF}, {3, 9}, {9.f, 9.f, 9.f, centre[0], centre[1], centre[2]}, {0, 0});
  g.EnableKeyFramePoints(192);
  std::vector<int32_t> row((size_t)N, -1), held;
  for (int i = 0; i < N; i++)
    if (hasPoint[(size_t)i]) { row[(size_t)i] = i; held.push_back(i); }
  g.SetPoints(held, std::vector<uint8_t>(held.size(), 0), std::vector<int32_t>(held.size(), 0));
  g.SetKeyFramePoints(KF, row);
  std::vector<int32_t> newSlot;
  for (int j = 0; j < N; j++) newSlot.push_back(N + (j * 7) % N);  // 7 and 150 are coprime: a permutation of N .. 2N - 1
  const MapPointTable::StereoPoints made = mp.CreateStereoPoints(&g, F, KF, pose, depth, 10.0f, ORBFE_STEREO_KEYFRAME, scale, newSlot, occupied, stale);
  print_ints("idx", made.idx); print_ints("slot", made.slot); print_ints("cleared", made.cleared);
  std::printf("walked=%d\n", made.walked);
  print_bits("positions", mp.Positions(made.slot));
  print_ints("descriptors", mp.Descriptors(made.slot));
  const MapPointTable::Projection pr = mp.ProjectInFrustum(made.slot, pose, -2.0f);
  print_ints("in_view", pr.mbTrackInView); print_ints("level", pr.mnTrackScaleLevel); print_bits("view_cos", pr.mTrackViewCos);

  // the temporal points of localisation mode: no graph
  MapPointTable vo(CAP);
  const MapPointTable::StereoPoints temp = vo.CreateStereoPoints(nullptr, F, 0, pose, depth, 10.0f, ORBFE_STEREO_TEMPORAL, scale, newSlot, occupied);
  print_ints("temporal_idx", temp.idx);
  print_bits("temporal_positions", vo.Positions(temp.slot));

  int threw = 0;
  auto refused = [&](int mode, const ObservationGraph* graph, int kf, const std::vector<int32_t>& slots, const std::vector<float>& z) {
    try {
      MapPointTable t(CAP);
      t.CreateStereoPoints(graph, F, kf, pose, z, 10.0f, mode, scale, slots, occupied);
    } catch (const std::exception&) { threw++; }
  };
  refused(ORBFE_STEREO_KEYFRAME, nullptr, KF, newSlot, depth);                 // no graph outside TEMPORAL
  refused(ORBFE_STEREO_KEYFRAME, &g, 1, newSlot, depth);                      // a kf slot never set
  refused(ORBFE_STEREO_KEYFRAME, &g, KF, newSlot, depth);                     // the new slots' rows are live by now
  refused(ORBFE_STEREO_TEMPORAL, nullptr, 0, {N, N + 1, N}, depth);           // a slot named twice
  refused(ORBFE_STEREO_TEMPORAL, nullptr, 0, {N, N + 1}, depth);              // more points than slots: capacity
  refused(ORBFE_STEREO_TEMPORAL, nullptr, 0, newSlot, std::vector<float>(N - 1, 1.0f));  // n is not the frame's
  std::printf("threw=%d\n", threw);
  return 0;
}
