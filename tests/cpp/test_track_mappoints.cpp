// orbfe_cpp::MapPointTable::ProjectLastFrame / SearchByProjectionLastFrame / ProjectKeyFrames / SearchByProjectionKeyFrames
// (include/orbfe_classes.hpp) on a world made by a formula tests/test_gpu_track_mappoints_cpp.py repeats: every input is exactly
// representable, so both sides hold the same bits.  Prints name=comma,separated,values.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

static const int P = 150, NKP = 300, K = 3;

template <typename T>
static void out(const char* name, const std::vector<T>& v) {
  std::printf("%s=", name);
  for (size_t i = 0; i < v.size(); i++) std::printf(i ? ",%d" : "%d", (int)v[i]);
  std::printf("\n");
}

int main() {
  std::vector<int32_t> slot(P), oct(P);
  std::vector<float> pos(3 * P), normal(3 * P), lo(P), hi(P), angle(P);
  std::vector<uint8_t> desc(32 * P), flags(P), skip(P);
  for (int i = 0; i < P; i++) {
    slot[i] = (i * 7) % 256;
    const float Z = 4.0f + (float)(i % 13);
    pos[3 * i] = (float)((i * 37) % 41 - 20) * 0.25f; pos[3 * i + 1] = (float)((i * 17) % 23 - 11) * 0.25f; pos[3 * i + 2] = i % 29 == 5 ? -Z : Z;
    normal[3 * i] = 0.0f; normal[3 * i + 1] = 0.0f; normal[3 * i + 2] = 1.0f;
    hi[i] = 2.0f * Z + (float)(i % 8); lo[i] = 0.125f * Z;
    flags[i] = (uint8_t)((i % 19 == 7 ? ORBFE_MP_BAD : 0) | (i % 5 ? ORBFE_MP_OBSERVED : 0));
    skip[i] = i % 23 == 3;
    oct[i] = i % 8;
    angle[i] = (float)((i * 11) % 360);
    for (int b = 0; b < 32; b++) desc[32 * i + b] = (uint8_t)((i * 7 + b * 13) & 255);
  }
  MapPointTable table(256);
  table.update(slot, pos, normal, lo, hi, desc, flags);

  std::vector<float> sf(8);
  sf[0] = 1.0f;
  for (int l = 1; l < 8; l++) sf[l] = sf[l - 1] * 1.25f;
  std::vector<orbfe_camera_pose> pose(K);
  for (int k = 0; k < K; k++) {
    orbfe_camera_pose& c = pose[k];
    c = orbfe_camera_pose{};
    c.Rcw[0] = c.Rcw[4] = c.Rcw[8] = 1.0f;
    c.tcw[0] = 0.015625f * (float)k; c.Ow[0] = -0.015625f * (float)k;
    c.fx = c.fy = 500.0f; c.cx = 320.0f; c.cy = 240.0f; c.mbf = 40.0f;
    c.min_x = 0.0f; c.max_x = 640.0f; c.min_y = 0.0f; c.max_y = 480.0f;
    c.log_scale_factor = 0.25f; c.n_levels = 8;
  }
  // the current frame: keypoint j sits on the pose-0 projection of point j % P (exact: fx / Z is representable or not, the
  // Python side repeats the float32 arithmetic), two pixels aside
  std::vector<KeyPoint> kps(NKP);
  std::vector<uint8_t> kd(32 * NKP);
  std::vector<float> ur(NKP);
  for (int j = 0; j < NKP; j++) {
    const int src = j % P;
    const float Z = std::fabs(pos[3 * src + 2]);
    kps[j] = KeyPoint{};
    kps[j].x = std::fmin(std::fmax((500.0f * pos[3 * src]) / Z + 320.0f + (float)(j % 3), 0.0f), 639.0f);
    kps[j].y = std::fmin(std::fmax((500.0f * pos[3 * src + 1]) / Z + 240.0f - (float)(j % 2), 0.0f), 479.0f);
    kps[j].octave = (src + 3 * (j / P)) % 8;
    kps[j].angle = (float)((src * 11 + 20) % 360);
    for (int b = 0; b < 32; b++) kd[32 * j + b] = (uint8_t)(((src * 7 + b * 13) & 255) ^ (b == j % 32 ? 1 : 0));
    ur[j] = j % 3 ? kps[j].x - 40.0f / Z : -1.0f;
  }
  FrameArrays cur(kps, kd, 0.0f, 640.0f, 0.0f, 480.0f, ur);
  cur.makeResident();

  const auto pl = table.ProjectLastFrame(slot, oct, pose[0], sf, 7.0f, 0, skip);
  out("last_valid", pl.valid);
  std::vector<int32_t> match;
  std::vector<uint8_t> valid;
  for (int mode = 0; mode < 3; mode++) {
    const int nm = table.SearchByProjectionLastFrame(cur, slot, oct, angle, pose[0], sf, 7.0f, mode, match, true, skip, {}, &valid);
    std::printf("last_n%d=%d\n", mode, nm);
    char name[32];
    std::snprintf(name, sizeof name, "last_match%d", mode);
    out(name, match);
  }
  out("last_searched", valid);

  const std::vector<int32_t> offsets = {0, 60, 60, P};  // (the middle job is empty)
  const auto pk = table.ProjectKeyFrames(offsets, slot, pose, skip);
  out("kf_valid", pk.valid);
  out("kf_level", pk.level);
  const std::vector<int32_t> nMatches =
      table.SearchByProjectionKeyFrames(cur, offsets, slot, angle, pose, sf, {10.0f, 3.0f, 10.0f}, {100, 64, 100}, match, true, skip);
  out("kf_n", nMatches);
  out("kf_match", match);

  int threw = 0;
  auto refused = [&](auto&& call) {
    try { call(); } catch (const std::exception&) { threw++; }
  };
  std::vector<int32_t> badSlot = slot, badOct = oct;
  badSlot[3] = 256;
  badOct[P - 1] = 8;
  refused([&] { table.ProjectLastFrame(badSlot, oct, pose[0], sf, 7.0f); });
  refused([&] { table.SearchByProjectionLastFrame(cur, slot, badOct, angle, pose[0], sf, 7.0f, 0, match); });
  refused([&] { table.SearchByProjectionLastFrame(cur, slot, oct, angle, pose[0], sf, 7.0f, 3, match); });
  refused([&] { table.ProjectKeyFrames({0, 60, 50, P}, slot, pose); });
  refused([&] { table.SearchByProjectionKeyFrames(cur, offsets, badSlot, angle, pose, sf, {10.0f, 3.0f, 10.0f}, {100, 64, 100}, match); });
  refused([&] { table.SearchByProjectionKeyFrames(cur, offsets, slot, angle, pose, sf, {10.0f}, {100}, match); });
  std::printf("threw=%d\n", threw);
  return 0;
}
