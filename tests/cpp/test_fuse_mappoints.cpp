// orbfe_cpp::MapPointTable::Fuse (include/orbfe_classes.hpp) on a world made by a formula tests/test_gpu_fuse_mappoints_cpp.py
// repeats: every input is exactly representable, so both sides hold the same bits.  Prints name=comma,separated,values.
#include <cmath>
#include <cstdio>
#include <stdexcept>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

static const int P = 120, NKP = 600, K = 3, KFCAP = 8;

template <typename T>
static void out(const char* name, const std::vector<T>& v) {
  std::printf("%s=", name);
  for (size_t i = 0; i < v.size(); i++) std::printf(i ? ",%d" : "%d", (int)v[i]);
  std::printf("\n");
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

  std::vector<float> sf(8), isig(8);
  sf[0] = 1.0f;
  for (int l = 1; l < 8; l++) sf[l] = sf[l - 1] * 1.25f;
  for (int l = 0; l < 8; l++) isig[l] = 1.0f / (sf[l] * sf[l]);
  std::vector<orbfe_camera_pose> pose(K);
  std::vector<FrameArrays*> frames;
  std::vector<const FrameArrays*> views;
  for (int k = 0; k < K; k++) {
    orbfe_camera_pose& c = pose[k];
    c = orbfe_camera_pose{};
    c.Rcw[0] = c.Rcw[4] = c.Rcw[8] = 1.0f;
    c.tcw[0] = 0.5f * (float)k; c.Ow[0] = -0.5f * (float)k;
    c.fx = c.fy = 500.0f; c.cx = 320.0f; c.cy = 240.0f; c.mbf = 40.0f;
    c.min_x = 0.0f; c.max_x = 640.0f; c.min_y = 0.0f; c.max_y = 480.0f;
    c.log_scale_factor = 0.25f; c.n_levels = 8;
    std::vector<KeyPoint> kps(NKP);
    std::vector<uint8_t> kd(32 * NKP);
    std::vector<float> ur;
    for (int j = 0; j < NKP; j++) {
      kps[j] = KeyPoint{};
      kps[j].x = (float)((j * 53 + k * 11) % 640); kps[j].y = (float)((j * 29 + k * 5) % 480); kps[j].octave = (j + k) % 8;
      const int src = j % P;
      for (int b = 0; b < 32; b++) kd[32 * j + b] = (uint8_t)(((src * 7 + b * 13) & 255) ^ (b == j % 32 ? 1 : 0));
      if (k == 1) ur.push_back(j % 3 ? kps[j].x - 8.0f : -1.0f);
    }
    frames.push_back(new FrameArrays(kps, kd, 0.0f, 640.0f, 0.0f, 480.0f, ur));
    if (k != 2) frames.back()->makeResident();
    views.push_back(frames.back());
  }
  std::vector<uint8_t> skip(K * P, 0), projected;
  for (int i = 0; i < K * P; i++) skip[i] = i % 23 == 3;

  out("gated", table.Fuse(views, pose, slot, sf, isig, 40.0f, true, nullptr, {}, skip, &projected));
  out("projected", projected);
  out("ungated", table.Fuse(views, pose, slot, sf, {}, 40.0f, false, nullptr, {}, skip));

  ObservationGraph graph(128, KFCAP, 8);
  std::vector<int32_t> kfSlot = {5, 2, 6};
  graph.SetKeyFrames({5, 2, 6}, {105, 102, 106}, std::vector<float>(9, 0.0f), {0, 0, 0});
  std::vector<int32_t> os, ok;
  std::vector<uint16_t> oi;
  std::vector<uint8_t> oo, ost;
  for (int i = 0; i < P; i++)
    if (i % 5 == 1) { os.push_back(slot[i]); ok.push_back(kfSlot[i % 3]); oi.push_back((uint16_t)i); oo.push_back(0); ost.push_back(0); }
  graph.SetPoints(os, std::vector<uint8_t>(os.size(), 0), std::vector<int32_t>(os.size(), -1));
  graph.AddObservations(os, ok, oi, oo, ost);
  out("graph", table.Fuse(views, pose, slot, sf, {}, 40.0f, false, &graph, kfSlot, {}, &projected));
  out("graph_projected", projected);

  int threw = 0;
  auto refused = [&](auto&& call) {
    try { call(); } catch (const std::exception&) { threw++; }
  };
  std::vector<int32_t> badSlot = slot;
  badSlot[3] = 128;
  refused([&] { table.Fuse(views, pose, badSlot, sf, isig); });
  refused([&] { table.Fuse(views, pose, slot, sf, isig, 3.0f, true, &graph, {5, 2, KFCAP}); });
  refused([&] { table.Fuse(views, {pose[0]}, slot, sf, isig); });
  refused([&] { table.Fuse(views, pose, slot, sf, {}); });
  refused([&] { table.Fuse(std::vector<const FrameArrays*>(65, views[0]), std::vector<orbfe_camera_pose>(65, pose[0]), slot, sf, isig); });
  std::printf("threw=%d\n", threw);
  for (FrameArrays* f : frames) delete f;
  return 0;
}
