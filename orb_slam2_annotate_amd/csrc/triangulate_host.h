// triangulate_host.h -- the host side of orbfe_triangulate_matches* (triangulate.hip) that needs no device: the argument
// checks, the dense pair list and the outputs of a call without pairs.  Plain C++ without a HIP include, so
// tests/cpp/triangulate_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/orbfe.h"
#include "triangulate_math.h"

namespace orbfe {

constexpr int kTriHostMaxNeighbours = 64;
constexpr int kTriHostMaxKeypoints = 16384;  // the frame limit of include/orbfe.h

inline bool tri_view_ok(const orbfe_frame_view* f) {
  return f && f->n >= 0 && f->n <= kTriHostMaxKeypoints && (f->n == 0 || (f->x && f->y && f->octave));
}
inline bool tri_is_stereo(const orbfe_frame_view* f, int i) { return f->u_right && f->u_right[i] >= 0.0f; }

// NULL when what a call READS is fine, else what is wrong with it.  f1 / f2[k]: views with HOST arrays (of a resident
// frame: the handle's own).  Shared by orbfe_triangulate_matches* and orbfe_create_triangulated_points (tripoints.hip),
// whose outputs differ.
inline const char* triangulate_check_inputs(const orbfe_frame_view* f1, const orbfe_keyframe_camera* cam1, int K,
                                            const orbfe_frame_view* const* f2, const orbfe_keyframe_camera* cam2,
                                            const int32_t* match12, const float* scale_factors, const float* level_sigma2,
                                            int n_levels) {
  if (K < 0 || K > kTriHostMaxNeighbours) return "n_neighbours outside [0, 64]";
  if (!f1 || !cam1) return "NULL key frame";
  if (f1->n < 0 || f1->n > kTriHostMaxKeypoints) return "key frame 1 holds more than 16384 keypoints (or fewer than 0)";
  if (!tri_view_ok(f1)) return "NULL array in key frame 1";
  if (!scale_factors || !level_sigma2) return "NULL level table";
  if (n_levels <= 0 || n_levels > ORBFE_MAX_LEVELS) return "n_levels outside (0, ORBFE_MAX_LEVELS]";
  const int n1 = f1->n;
  if (K > 0 && (!f2 || !cam2)) return "NULL array";
  if (K > 0 && n1 > 0 && !match12) return "NULL array";
  for (int k = 0; k < K; k++) {
    const orbfe_frame_view* g = f2[k];
    if (!g) return "NULL neighbour";
    if (g->n < 0 || g->n > kTriHostMaxKeypoints) return "a neighbour holds more than 16384 keypoints (or fewer than 0)";
    if (!tri_view_ok(g)) return "NULL array in a neighbour";
    for (int i1 = 0; i1 < n1; i1++) {
      const int32_t i2 = match12[(size_t)k * n1 + i1];
      if (i2 < -1 || i2 >= g->n) return "match outside [-1, n2)";
      if (i2 < 0) continue;
      if (f1->octave[i1] < 0 || f1->octave[i1] >= n_levels || g->octave[i2] < 0 || g->octave[i2] >= n_levels)
        return "octave of a matched keypoint outside the level table";
      if (tri_is_stereo(f1, i1)) {
        if (!cam1->depth) return "key frame 1 has a matched stereo keypoint but no depth";
        if (!(cam1->depth[i1] > 0.0f)) return "depth of a matched stereo keypoint is not positive";
      }
      if (tri_is_stereo(g, i2)) {
        if (!cam2[k].depth) return "a neighbour has a matched stereo keypoint but no depth";
        if (!(cam2[k].depth[i2] > 0.0f)) return "depth of a matched stereo keypoint is not positive";
      }
    }
  }
  return nullptr;
}

// NULL when the arguments of orbfe_triangulate_matches* are fine, else what is wrong with them.  winner is only looked at
// when wantWinner (the multi form).
inline const char* triangulate_check(const orbfe_frame_view* f1, const orbfe_keyframe_camera* cam1, int K,
                                     const orbfe_frame_view* const* f2, const orbfe_keyframe_camera* cam2,
                                     const int32_t* match12, const float* scale_factors, const float* level_sigma2,
                                     int n_levels, const float* x3d, const uint8_t* status, const int32_t* n_created,
                                     const int32_t* winner, bool wantWinner) {
  if (const char* e = triangulate_check_inputs(f1, cam1, K, f2, cam2, match12, scale_factors, level_sigma2, n_levels)) return e;
  const int n1 = f1->n;
  if (wantWinner && n1 > 0 && !winner) return "NULL winner";
  if (K > 0 && !n_created) return "NULL array";
  if (K > 0 && n1 > 0 && (!x3d || !status)) return "NULL array";
  return nullptr;
}

// the arguments have passed triangulate_check: every match of match12, neighbour by neighbour, keypoint by keypoint
inline void triangulate_pairs(const orbfe_frame_view* f1, const orbfe_keyframe_camera* cam1, int K,
                              const orbfe_frame_view* const* f2, const orbfe_keyframe_camera* cam2, const int32_t* match12,
                              std::vector<TriangulatePair>* out) {
  out->clear();
  const int n1 = f1->n;
  for (int k = 0; k < K; k++)
    for (int i1 = 0; i1 < n1; i1++) {
      const int32_t i2 = match12[(size_t)k * n1 + i1];
      if (i2 < 0) continue;
      const orbfe_frame_view* g = f2[k];
      TriangulatePair p;
      p.k = k; p.i1 = i1; p.i2 = i2;
      p.depth1 = tri_is_stereo(f1, i1) ? cam1->depth[i1] : 0.0f;
      p.depth2 = tri_is_stereo(g, i2) ? cam2[k].depth[i2] : 0.0f;
      p.xraw1 = cam1->x_raw ? cam1->x_raw[i1] : f1->x[i1];
      p.yraw1 = cam1->y_raw ? cam1->y_raw[i1] : f1->y[i1];
      p.xraw2 = cam2[k].x_raw ? cam2[k].x_raw[i2] : g->x[i2];
      p.yraw2 = cam2[k].y_raw ? cam2[k].y_raw[i2] : g->y[i2];
      out->push_back(p);
    }
}

inline TriCamera tri_camera(const orbfe_keyframe_camera* c) {
  TriCamera t;
  memcpy(t.Tcw, c->Tcw, sizeof t.Tcw);
  memcpy(t.Ow, c->Ow, sizeof t.Ow);
  t.fx = c->fx; t.fy = c->fy; t.cx = c->cx; t.cy = c->cy; t.invfx = c->invfx; t.invfy = c->invfy; t.mb = c->mb; t.mbf = c->mbf;
  return t;
}

// what a call without a pair returns (and what every slot without a match holds after any call)
inline void triangulate_init_outputs(int K, int n1, float* x3d, uint8_t* status, int32_t* n_created, int32_t* winner) {
  const size_t slots = (size_t)(K > 0 ? K : 0) * (size_t)n1;
  if (slots) {
    memset(x3d, 0, slots * 3 * sizeof(float));
    memset(status, 0, slots);
  }
  for (int k = 0; k < K; k++) n_created[k] = 0;
  if (winner)
    for (int i = 0; i < n1; i++) winner[i] = -1;
}

}  // namespace orbfe
