// stereopoints_host.h -- where stereo and RGB-D map points are born (include/orbfe.h: orbfe_stereo_points_select,
// orbfe_count_close_points; device side: stereopoints.hip, k_stereopoints.hip).  Plain C++ without a HIP include; the
// kernel takes sp_candidate, sp_unproject and sp_normal_range from here, so host and device share one definition.
// References: Tracking::StereoInitialization (src/Tracking.cc:563-578), Tracking::UpdateLastFrame (:899-949),
// Tracking::CreateNewKeyFrame (:1182-1234), Tracking::NeedNewKeyFrame (:1100-1114), Frame::UnprojectStereo
// (src/Frame.cc:713-727), the Frame constructor of MapPoint (src/MapPoint.cc:46-71) and MapPoint::UpdateNormalAndDepth
// (src/MapPoint.cc:360-404) for a row of one entry.
//
// `mRwc * x3Dc + mOw` is one cv::gemm with beta = 1 over CV_32F operands: the double-accumulator restatement of
// loopcorrect_host.h (include/orbfe.h, loop correction), D_i = (float)((double)A_i0 x + (double)A_i1 y + (double)A_i2 z +
// (double)C_i), added left to right.  As there, no copy of OpenCV's matmul.cpp was at hand to check its small-matrix path
// against this.
#pragma once
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../../include/orbfe.h"
#include "g2o_math.h"

namespace orbfe {

constexpr int kStereoMaxKeypoints = 16384;  // as the triangulation call caps a frame
constexpr int kStereoMinWalk = 100;         // "if there are less than 100 close points we create the 100 closest"

// z > 0 on the bits: positive (sub)normals and +inf; zero, negatives and every NaN are no candidates (:1187)
ORBFE_HD inline bool sp_candidate(uint32_t zbits) { return zbits - 1u < 0x7f800000u; }
inline uint32_t sp_bits(float z) {
  uint32_t b;
  memcpy(&b, &z, 4);
  return b;
}

// Frame::UnprojectStereo (src/Frame.cc:718-723).  Rwc is the transpose of pose.Rcw, read in place
ORBFE_HD inline void sp_unproject(const orbfe_camera_pose& p, float invfx, float invfy, float u, float v, float z, float P[3]) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float x = __fmul_rn(__fmul_rn(__fsub_rn(u, p.cx), z), invfx), y = __fmul_rn(__fmul_rn(__fsub_rn(v, p.cy), z), invfy);
#else
  const float x = ((u - p.cx) * z) * invfx, y = ((v - p.cy) * z) * invfy;
#endif
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double s = (double)p.Rcw[r] * (double)x;  // (a product of two binary32 values is exact in binary64)
    s += (double)p.Rcw[3 + r] * (double)y;
    s += (double)p.Rcw[6 + r] * (double)z;
    s += (double)p.Ow[r];
    P[r] = (float)s;
  }
}

// MapPoint::UpdateNormalAndDepth for a row of one entry, the entry being the reference key frame (and, with C = the
// frame's Ow, :53-64 of the Frame constructor): orbfe_obsgraph_update_normal_depth's restatement, operation by operation
ORBFE_HD inline void sp_normal_range(const float P[3], const float C[3], float levelScale, float topScale, float nrmOut[3], float* minDist,
                                     float* maxDist) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float dx = __fsub_rn(P[0], C[0]), dy = __fsub_rn(P[1], C[1]), dz = __fsub_rn(P[2], C[2]);
  const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
  const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz)));
  const float a = (float)__ddiv_rn(1.0, nrm), one = (float)__ddiv_rn(1.0, 1.0);
  nrmOut[0] = __fmul_rn(__fadd_rn(0.0f, __fmul_rn(dx, a)), one);
  nrmOut[1] = __fmul_rn(__fadd_rn(0.0f, __fmul_rn(dy, a)), one);
  nrmOut[2] = __fmul_rn(__fadd_rn(0.0f, __fmul_rn(dz, a)), one);
  const float hi = __fmul_rn((float)nrm, levelScale);
  *maxDist = hi;
  *minDist = __fdiv_rn(hi, topScale);
#else
  const float dx = P[0] - C[0], dy = P[1] - C[1], dz = P[2] - C[2];
  const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
  const double nrm = sqrt((ddx * ddx + ddy * ddy) + ddz * ddz);
  const float a = (float)(1.0 / nrm), one = (float)(1.0 / 1.0);
  nrmOut[0] = (0.0f + dx * a) * one;
  nrmOut[1] = (0.0f + dy * a) * one;
  nrmOut[2] = (0.0f + dz * a) * one;
  const float hi = (float)nrm * levelScale;
  *maxDist = hi;
  *minDist = hi / topScale;
#endif
}

template <typename T>
inline bool sp_finite(const T* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!isfinite((double)v[i])) return false;
  return true;
}

// what the pose must be before anything is computed from it
inline const char* sp_check_pose(const orbfe_camera_pose* p) {
  if (!p) return "NULL pose";
  if (!sp_finite(p->Rcw, 9) || !sp_finite(p->Ow, 3) || !sp_finite(&p->fx, 4)) return "the pose is not finite";
  if (p->fx == 0.0f || p->fy == 0.0f) return "fx and fy must not be 0";
  return nullptr;
}

// the operands both forms share: NULL when they are fine.  occupied / stale may be NULL (none set)
inline const char* sp_check_operands(int n, const int32_t* octave, const float* depth, const uint8_t* occupied, const uint8_t* stale,
                                     const orbfe_camera_pose* pose, int mode, const float* scale, int nLevels) {
  if (n < 0) return "negative count";
  if (n > kStereoMaxKeypoints) return "more than 16384 keypoints";
  if (mode != ORBFE_STEREO_ALL && mode != ORBFE_STEREO_KEYFRAME && mode != ORBFE_STEREO_TEMPORAL) return "unknown mode";
  if (nLevels < 1 || nLevels > 256) return "n_levels must be 1 .. 256";
  if (!scale) return "NULL scale_factors";
  if (const char* e = sp_check_pose(pose)) return e;
  if (n > 0 && (!octave || !depth)) return "NULL array";
  for (int i = 0; i < n; i++)
    if (octave[i] < 0 || octave[i] >= nLevels) return "a keypoint's octave is not below n_levels";
  if (mode != ORBFE_STEREO_ALL && occupied && stale)
    for (int i = 0; i < n; i++)
      if (occupied[i] && stale[i]) return "a keypoint is both occupied and stale";
  return nullptr;
}

// The walk (:1182-1233, :899-949; ALL: :563-578).  order: the candidates' keypoint indices as they are visited, the
// first *walked of them handled; created[j] = 1 when visit j makes a point.  Returns the number created.
inline int sp_walk(int n, const float* depth, const uint8_t* occupied, float thDepth, int mode, std::vector<int32_t>* order,
                   std::vector<uint8_t>* created, int* walked) {
  std::vector<std::pair<float, int>> cand;
  cand.reserve((size_t)n);
  for (int i = 0; i < n; i++)
    if (sp_candidate(sp_bits(depth[i]))) cand.emplace_back(depth[i], i);
  if (mode != ORBFE_STEREO_ALL) std::sort(cand.begin(), cand.end());  // pair<float, int>: by z, ties by i (:1195)
  order->clear();
  created->clear();
  int nCreated = 0, nPoints = 0;
  for (size_t j = 0; j < cand.size(); j++) {
    const int i = cand[j].second;
    const bool make = mode == ORBFE_STEREO_ALL || !(occupied && occupied[i]);  // !pMP || Observations() < 1 (:1205-1211)
    order->push_back(i);
    created->push_back(make ? 1 : 0);
    nCreated += make ? 1 : 0;
    nPoints++;  // in either branch (:1224, :1228)
    if (mode != ORBFE_STEREO_ALL && cand[j].first > thDepth && nPoints > kStereoMinWalk) break;  // (:1231)
  }
  *walked = nPoints;
  return nCreated;
}

// orbfe_stereo_points_select.  *over: more points are created than `capacity` (*nCreated and *nWalked set, no array
// written).  NULL when done, else what is wrong (nothing written)
inline const char* stereo_points_select(int n, const float* x, const float* y, const int32_t* octave, const float* depth,
                                        const uint8_t* occupied, const uint8_t* stale, const orbfe_camera_pose* pose, float thDepth, int mode,
                                        const float* scale, int nLevels, const float* centre, int capacity, int32_t* createdIdx, float* pos,
                                        float* normal, float* minDist, float* maxDist, uint8_t* cleared, int32_t* nCreated, int32_t* nWalked,
                                        bool* over) {
  *over = false;
  if (!nCreated || !nWalked) return "NULL count";
  if (capacity < 0) return "negative capacity";
  if (const char* e = sp_check_operands(n, octave, depth, occupied, stale, pose, mode, scale, nLevels)) return e;
  if (n > 0 && (!x || !y)) return "NULL array";
  if (!centre || !sp_finite(centre, 3)) return "the camera centre is missing or not finite";
  if (capacity > 0 && (!createdIdx || !pos || !normal || !minDist || !maxDist)) return "NULL output array";
  std::vector<int32_t> order;
  std::vector<uint8_t> made;
  int walked = 0;
  const int count = sp_walk(n, depth, occupied, thDepth, mode, &order, &made, &walked);
  *nCreated = count;
  *nWalked = walked;
  if (count > capacity) {
    *over = true;
    return "more points are created than `capacity` (see *n_created)";
  }
  if (cleared)
    for (int i = 0; i < n; i++) cleared[i] = 0;
  const float invfx = 1.0f / pose->fx, invfy = 1.0f / pose->fy;  // Frame::invfx, invfy
  int w = 0;
  for (int j = 0; j < walked; j++) {
    if (!made[(size_t)j]) continue;
    const int i = order[(size_t)j];
    float* P = pos + 3 * (size_t)w;
    sp_unproject(*pose, invfx, invfy, x[i], y[i], depth[i], P);
    sp_normal_range(P, centre, scale[octave[i]], scale[nLevels - 1], normal + 3 * (size_t)w, minDist + w, maxDist + w);
    createdIdx[w] = i;
    if (cleared && mode == ORBFE_STEREO_KEYFRAME && stale && stale[i]) cleared[i] = 1;  // mvpMapPoints[i] = NULL (:1207-1211)
    w++;
  }
  return nullptr;
}

// nTrackedClose / nNonTrackedClose of Tracking::NeedNewKeyFrame (:1100-1114)
inline const char* count_close_points(int n, const float* depth, const uint8_t* hasPoint, const uint8_t* outlier, float thDepth, int32_t* tracked,
                                      int32_t* nonTracked) {
  if (n < 0) return "negative count";
  if (!tracked || !nonTracked) return "NULL count";
  if (n > 0 && (!depth || !hasPoint || !outlier)) return "NULL array";
  int t = 0, u = 0;
  for (int i = 0; i < n; i++) {
    if (!(depth[i] > 0 && depth[i] < thDepth)) continue;
    if (hasPoint[i] && !outlier[i]) t++;
    else u++;
  }
  *tracked = t;
  *nonTracked = u;
  return nullptr;
}

}  // namespace orbfe
