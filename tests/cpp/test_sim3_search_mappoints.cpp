// orbfe_cpp::MapPointTable::SearchBySim3 / SearchByProjection (include/orbfe_classes.hpp) on a world made by a formula
// tests/test_gpu_sim3_search_cpp.py repeats: every input is exactly representable, so both sides hold the same bits.  Prints
// name=comma,separated,values.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

static const int P = 120, NKP = 600, K = 2;

template <typename T>
static void out(const char* name, const std::vector<T>& v) {
  std::printf("%s=", name);
  for (size_t i = 0; i < v.size(); i++) std::printf(i ? ",%d" : "%d", (int)v[i]);
  std::printf("\n");
}

static orbfe_sim3_leg leg(float twx, float tx) {
  orbfe_sim3_leg l{};
  l.Rw[0] = l.Rw[4] = l.Rw[8] = 1.0f;
  l.sR[0] = l.sR[4] = l.sR[8] = 1.0f;
  l.tw[0] = twx; l.t[0] = tx;
  l.fx = l.fy = 500.0f; l.cx = 320.0f; l.cy = 240.0f;
  l.min_x = 0.0f; l.max_x = 640.0f; l.min_y = 0.0f; l.max_y = 480.0f;
  l.log_scale_factor = 0.25f; l.n_levels = 8;
  return l;
}

int main() {
  std::vector<int32_t> slot(P);
  std::vector<float> pos(3 * P), normal(3 * P), lo(P), hi(P);
  std::vector<uint8_t> desc(32 * P), flags(P);
  for (int i = 0; i < P; i++) {
    slot[i] = (i * 7) % 128;
    const float Z = 4.0f + (float)(i % 13);
    pos[3 * i] = (float)((i * 37) % 41 - 20) * 0.25f; pos[3 * i + 1] = (float)((i * 17) % 23 - 11) * 0.25f; pos[3 * i + 2] = Z;
    normal[3 * i] = 0.0f; normal[3 * i + 1] = 0.0f; normal[3 * i + 2] = 1.0f;
    hi[i] = 2.0f * Z + (float)(i % 8); lo[i] = 0.125f * Z;
    flags[i] = i % 19 == 7 ? ORBFE_MP_BAD : 0;
    for (int b = 0; b < 32; b++) desc[32 * i + b] = (uint8_t)((i * 7 + b * 13) & 255);
  }
  MapPointTable table(128);
  table.update(slot, pos, normal, lo, hi, desc, flags);

  std::vector<float> sf(8);
  sf[0] = 1.0f;
  for (int l = 1; l < 8; l++) sf[l] = sf[l - 1] * 1.25f;
  std::vector<FrameArrays*> frames;
  for (int k = 0; k < K + 1; k++) {  // frame 0 is KF1, frames 1 .. K the candidates
    std::vector<KeyPoint> kps(NKP);
    std::vector<uint8_t> kd(32 * NKP);
    for (int j = 0; j < NKP; j++) {
      kps[j] = KeyPoint{};
      kps[j].x = (float)((j * 53 + k * 11) % 640); kps[j].y = (float)((j * 29 + k * 5) % 480); kps[j].octave = (j + (k > 0 ? 1 : 0)) % 8;
      if (j < P) {  // the first P keypoints of every frame sit on the projection of point j, where it is inside: KF1 and candidate 0
                    // share a camera, candidate 1 stands half a unit along x (c2 = P + (0.5, 0, 0), exact in binary32)
        const float shift = k == 2 ? 0.5f : 0.0f;
        const float u = 500.0f * ((pos[3 * j] + shift) / pos[3 * j + 2]) + 320.0f, v = 500.0f * (pos[3 * j + 1] / pos[3 * j + 2]) + 240.0f;
        if (u >= 0.0f && u < 640.0f && v >= 0.0f && v < 480.0f) { kps[j].x = u; kps[j].y = v; }
      }
      const int src = j % P;
      for (int b = 0; b < 32; b++) kd[32 * j + b] = (uint8_t)(((src * 7 + b * 13) & 255) ^ (b == j % 32 ? 1 : 0));
    }
    frames.push_back(new FrameArrays(kps, kd, 0.0f, 640.0f, 0.0f, 480.0f, {}));
    if (k != 2) frames.back()->makeResident();
  }
  std::vector<int32_t> slot1(NKP), slot2(K * NKP), offsets2 = {0, NKP, 2 * NKP}, matchedIn(K * NKP, -1);
  std::vector<uint8_t> already2(K * NKP, 0);
  for (int j = 0; j < NKP; j++) slot1[j] = j % 4 == 0 ? -1 : slot[j % P];
  for (int k = 0; k < K; k++)
    for (int j = 0; j < NKP; j++) {
      slot2[k * NKP + j] = j % 5 == 0 ? -1 : slot[j < P ? j : (j * 3 + k) % P];
      if (j % 17 == 2) matchedIn[k * NKP + j] = slot[(j + k) % P];
      already2[k * NKP + j] = j % 13 == 1;
    }
  std::vector<orbfe_sim3_leg> legs12 = {leg(0.0f, 0.0f), leg(0.0f, 0.5f)}, legs21 = {leg(0.0f, 0.0f), leg(0.5f, -0.5f)};
  std::vector<const FrameArrays*> KF2s = {frames[1], frames[2]};
  std::vector<int32_t> match12;
  out("found", table.SearchBySim3(*frames[0], slot1, KF2s, offsets2, slot2, legs12, legs21, sf, sf, 40.0f, match12));
  out("match12", match12);
  out("found_masked", table.SearchBySim3(*frames[0], slot1, KF2s, offsets2, slot2, legs12, legs21, sf, sf, 40.0f, match12, matchedIn, nullptr,
                                         {}, already2));
  out("match12_masked", match12);

  orbfe_camera_pose c{};
  c.Rcw[0] = c.Rcw[4] = c.Rcw[8] = 1.0f;
  c.tcw[0] = 0.5f; c.Ow[0] = -0.5f;
  c.fx = c.fy = 500.0f; c.cx = 320.0f; c.cy = 240.0f; c.mbf = 40.0f;
  c.min_x = 0.0f; c.max_x = 640.0f; c.min_y = 0.0f; c.max_y = 480.0f;
  c.log_scale_factor = 0.25f; c.n_levels = 8;
  std::vector<uint8_t> matched(NKP, 0), skip(P, 0), projected;
  for (int j = 0; j < NKP; j++) matched[j] = j % 7 == 3;
  for (int i = 0; i < P; i++) skip[i] = i % 23 == 3;
  std::vector<int32_t> match;
  const int n = table.SearchByProjection(*frames[1], c, slot, sf, 40.0f, match, matched, skip, &projected);
  out("projection", match);
  out("projection_projected", projected);
  std::printf("projection_n=%d\n", n);

  int threw = 0;
  auto refused = [&](auto&& call) {
    try { call(); } catch (const std::exception&) { threw++; }
  };
  std::vector<int32_t> bad1 = slot1, badSlot = slot;
  bad1[3] = 128;
  badSlot[3] = -1;
  refused([&] { table.SearchBySim3(*frames[0], bad1, KF2s, offsets2, slot2, legs12, legs21, sf, sf, 40.0f, match12); });
  refused([&] { table.SearchBySim3(*frames[0], slot1, KF2s, {0, NKP}, slot2, legs12, legs21, sf, sf, 40.0f, match12); });
  refused([&] { table.SearchBySim3(*frames[0], slot1, KF2s, offsets2, slot2, {legs12[0]}, legs21, sf, sf, 40.0f, match12); });
  refused([&] { table.SearchByProjection(*frames[1], c, badSlot, sf, 40.0f, match); });
  refused([&] { table.SearchByProjection(*frames[1], c, slot, sf, 40.0f, match, {1, 0}); });
  std::printf("threw=%d\n", threw);
  for (FrameArrays* f : frames) delete f;
  return 0;
}
