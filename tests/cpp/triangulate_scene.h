// Reader of the scene files tests/triangulate_ref.py writes (write_scene): whitespace-separated numbers, floats as their
// float32 bit patterns in hex.  Shared by triangulate_cpu.cpp and test_triangulate.cpp.
#pragma once
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbfe.h"

struct TriSceneFrame {
  int n = 0;
  bool stereo = false, raw = false;
  std::vector<float> x, y, ur, depth, xraw, yraw;
  std::vector<int32_t> octave;
  orbfe_keyframe_camera cam = {};
  orbfe_frame_view view = {};
};
struct TriScene {
  int K = 0, n1 = 0, nLevels = 0;
  std::vector<float> scaleFactors, levelSigma2;
  float ratioFactor = 0.0f;
  std::vector<TriSceneFrame> frames;  // key frame 1, then the neighbours
  std::vector<int32_t> match12;
  std::vector<const orbfe_frame_view*> views2;
  std::vector<orbfe_keyframe_camera> cams2;
};

inline bool tri_read_floats(FILE* f, float* out, size_t n) {
  for (size_t i = 0; i < n; i++) {
    unsigned bits;
    if (std::fscanf(f, "%x", &bits) != 1) return false;
    const uint32_t b = bits;
    std::memcpy(out + i, &b, 4);
  }
  return true;
}
inline bool tri_read_floats(FILE* f, std::vector<float>* out, size_t n) {
  out->resize(n);
  return tri_read_floats(f, out->data(), n);
}
inline bool tri_read_ints(FILE* f, std::vector<int32_t>* out, size_t n) {
  out->resize(n);
  for (size_t i = 0; i < n; i++)
    if (std::fscanf(f, "%d", &(*out)[i]) != 1) return false;
  return true;
}

inline bool tri_read_scene(const char* path, TriScene* S) {
  FILE* f = std::fopen(path, "r");
  if (!f) return false;
  bool ok = std::fscanf(f, "%d %d %d", &S->K, &S->n1, &S->nLevels) == 3;
  ok = ok && tri_read_floats(f, &S->scaleFactors, (size_t)S->nLevels) && tri_read_floats(f, &S->levelSigma2, (size_t)S->nLevels) &&
       tri_read_floats(f, &S->ratioFactor, 1);
  S->frames.resize(ok ? (size_t)S->K + 1 : 0);
  for (TriSceneFrame& F : S->frames) {
    int st = 0, raw = 0;
    float k8[8];
    ok = ok && std::fscanf(f, "%d %d %d", &F.n, &st, &raw) == 3;
    if (!ok) break;
    F.stereo = st != 0; F.raw = raw != 0;
    const size_t n = (size_t)F.n;
    ok = tri_read_floats(f, F.cam.Tcw, 12) && tri_read_floats(f, F.cam.Ow, 3) && tri_read_floats(f, k8, 8) &&
         tri_read_floats(f, &F.x, n) && tri_read_floats(f, &F.y, n) && tri_read_ints(f, &F.octave, n);
    if (ok && F.stereo) ok = tri_read_floats(f, &F.ur, n) && tri_read_floats(f, &F.depth, n);
    if (ok && F.raw) ok = tri_read_floats(f, &F.xraw, n) && tri_read_floats(f, &F.yraw, n);
    F.cam.fx = k8[0]; F.cam.fy = k8[1]; F.cam.cx = k8[2]; F.cam.cy = k8[3]; F.cam.invfx = k8[4]; F.cam.invfy = k8[5];
    F.cam.mb = k8[6]; F.cam.mbf = k8[7];
  }
  ok = ok && tri_read_ints(f, &S->match12, (size_t)S->K * (size_t)S->n1);
  std::fclose(f);
  if (!ok) return false;
  for (TriSceneFrame& F : S->frames) {  // (pointers only now: the vectors no longer move)
    F.cam.depth = F.stereo ? F.depth.data() : nullptr;
    F.cam.x_raw = F.raw ? F.xraw.data() : nullptr;
    F.cam.y_raw = F.raw ? F.yraw.data() : nullptr;
    F.view.n = F.n; F.view.x = F.x.data(); F.view.y = F.y.data(); F.view.octave = F.octave.data();
    F.view.u_right = F.stereo ? F.ur.data() : nullptr;
    F.view.min_x = 0.0f; F.view.max_x = 640.0f; F.view.min_y = 0.0f; F.view.max_y = 480.0f;
  }
  for (int k = 0; k < S->K; k++) {
    S->views2.push_back(&S->frames[1 + k].view);
    S->cams2.push_back(S->frames[1 + k].cam);
  }
  return true;
}

// status [K * n1], x3d [K * n1 * 3] as bit patterns, then whatever integers the program appends
inline bool tri_write_result(const char* path, const std::vector<uint8_t>& status, const std::vector<float>& x3d,
                             const std::vector<int32_t>& rest) {
  FILE* f = std::fopen(path, "w");
  if (!f) return false;
  for (uint8_t s : status) std::fprintf(f, "%d ", (int)s);
  std::fprintf(f, "\n");
  for (float v : x3d) {
    uint32_t b;
    std::memcpy(&b, &v, 4);
    std::fprintf(f, "%08x ", b);
  }
  std::fprintf(f, "\n");
  for (int32_t v : rest) std::fprintf(f, "%d ", v);
  std::fprintf(f, "\n");
  return std::fclose(f) == 0;
}
