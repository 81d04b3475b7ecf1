// tripoints_host.h -- where the triangulated map points of LocalMapping::CreateNewMapPoints are born (include/orbfe.h:
// orbfe_triangulated_points_select; device side: tripoints.hip, k_tripoints.hip).  Plain C++ without a HIP include; the
// kernel takes tp_keep and tp_normal_range from here, so host and device share one definition.  The per-pair arithmetic
// (status and position) is tri_pair of triangulate_math.h, included and not restated.
// References: LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:283-501: the neighbour loop :283, the pair loop :333,
// the birth :484-500), ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:800-803: a keypoint that has a MapPoint is
// no longer searched), MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) and
// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:360-404), both for a row of two entries.
//
//   who       pair (k, i1) makes a point when its status is ORBFE_TRI_CREATED and k is the smallest neighbour index with a
//             CREATED pair for i1 (the `winner` of orbfe_triangulate_matches_multi): AddMapPoint(pMP, idx1) at :489 takes
//             i1 out of every later neighbour's search
//   order     ascending (k, i1): the neighbour loop outside, vMatchedIndices -- ascending in idx1 -- inside
//   position  the pair's x3d, as it is
//   descriptor  with two observations every median of :306-321 is a self-distance 0, `median < BestMedian` is strict, so
//             the first entry of the row wins: the key frame with the smaller mnId in the ascending-mnId row.  This is
//             orbfe_obsgraph_distinctive_descriptors for a row of two entries; desc_from says which frame's row it is
//   normal    orbfe_obsgraph_update_normal_depth for a row of two entries A, B in ascending mnId, operation by operation:
//             d = P - C, a = (float)(1.0 / sqrt(sum (double)d_i^2)); normal_i = ((0.0f + dA_i * aA) + dB_i * aB) *
//             (float)(1.0 / 2)
//   range     the reference key frame is key frame 1 (mpRefKF = mpCurrentKeyFrame, :484): dist = (float)|P - C1|,
//             max_dist = dist * scale_factors[octave1[i1]], min_dist = max_dist / scale_factors[n_levels - 1]
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "../../include/orbfe.h"
#include "triangulate_host.h"
#include "triangulate_math.h"

namespace orbfe {

// does pair (k, i1) with this status make a point?  winner: the smallest k with a CREATED pair for i1
ORBFE_HD inline bool tp_keep(int status, int k, int winner) { return status == kTriCreated && winner == k; }

// one entry's term of MapPoint::UpdateNormalAndDepth (:381-385): t = normali / cv::norm(normali), *len = (float)norm
ORBFE_HD inline void tp_term(const float P[3], const float C[3], float t[3], float* len) {
#if defined(__HIP_DEVICE_COMPILE__)
  const float dx = __fsub_rn(P[0], C[0]), dy = __fsub_rn(P[1], C[1]), dz = __fsub_rn(P[2], C[2]);
  const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
  const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz)));
  const float a = (float)__ddiv_rn(1.0, nrm);  // Mat / double: the matrix times (float)(1 / s)
  t[0] = __fmul_rn(dx, a); t[1] = __fmul_rn(dy, a); t[2] = __fmul_rn(dz, a);
#else
  const float dx = P[0] - C[0], dy = P[1] - C[1], dz = P[2] - C[2];
  const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
  const double nrm = sqrt((ddx * ddx + ddy * ddy) + ddz * ddz);
  const float a = (float)(1.0 / nrm);
  t[0] = dx * a; t[1] = dy * a; t[2] = dz * a;
#endif
  *len = (float)nrm;
}

// UpdateNormalAndDepth for the row {key frame 1, neighbour}: C1 / C2 their centres, firstIs2 = the neighbour's mnId is the
// smaller one (it stands first in the row), the reference key frame is key frame 1
ORBFE_HD inline void tp_normal_range(const float P[3], const float C1[3], const float C2[3], bool firstIs2, float levelScale, float topScale,
                                     float nrmOut[3], float* minDist, float* maxDist) {
  float t1[3], t2[3], len1, len2;
  tp_term(P, C1, t1, &len1);
  tp_term(P, C2, t2, &len2);
  (void)len2;
#if defined(__HIP_DEVICE_COMPILE__)
  const float half = (float)__ddiv_rn(1.0, 2.0);  // normal / n (:402)
#pragma unroll
  for (int r = 0; r < 3; r++) {
    const float a = firstIs2 ? t2[r] : t1[r], b = firstIs2 ? t1[r] : t2[r];
    nrmOut[r] = __fmul_rn(__fadd_rn(__fadd_rn(0.0f, a), b), half);
  }
  const float hi = __fmul_rn(len1, levelScale);
  *maxDist = hi;
  *minDist = __fdiv_rn(hi, topScale);
#else
  const float half = (float)(1.0 / 2.0);
  for (int r = 0; r < 3; r++) {
    const float a = firstIs2 ? t2[r] : t1[r], b = firstIs2 ? t1[r] : t2[r];
    nrmOut[r] = ((0.0f + a) + b) * half;
  }
  const float hi = len1 * levelScale;
  *maxDist = hi;
  *minDist = hi / topScale;
#endif
}

inline bool tp_finite3(const float* v) { return isfinite(v[0]) && isfinite(v[1]) && isfinite(v[2]); }

// a keypoint of neighbour k named by two matches of match12's row k?  n2: an upper bound of the row's entries
inline bool tp_i2_twice(int n1, const int32_t* row, int n2, std::vector<uint8_t>* seen) {
  seen->assign((size_t)n2, 0);
  for (int i1 = 0; i1 < n1; i1++) {
    const int32_t i2 = row[i1];
    if (i2 < 0) continue;
    if ((*seen)[(size_t)i2]) return true;
    (*seen)[(size_t)i2] = 1;
  }
  return false;
}

// the pairs that make a point, in creation order: ascending (k, i1)
inline int tp_walk(int n1, int K, const uint8_t* status, std::vector<int32_t>* ks, std::vector<int32_t>* i1s) {
  std::vector<int32_t> winner((size_t)n1, INT32_MAX);
  for (int k = K - 1; k >= 0; k--)
    for (int i1 = 0; i1 < n1; i1++)
      if (status[(size_t)k * n1 + i1] == kTriCreated) winner[(size_t)i1] = k;
  ks->clear();
  i1s->clear();
  for (int k = 0; k < K; k++)
    for (int i1 = 0; i1 < n1; i1++)
      if (tp_keep(status[(size_t)k * n1 + i1], k, winner[(size_t)i1])) {
        ks->push_back(k);
        i1s->push_back(i1);
      }
  return (int)ks->size();
}

// orbfe_triangulated_points_select.  *over: more points are created than `capacity` (*nCreated set, no array written).
// NULL when done, else what is wrong (nothing written)
inline const char* triangulated_points_select(int n1, int K, const int32_t* match12, const uint8_t* status, const float* x3d, int64_t kf1Id,
                                              const int64_t* kf2Id, const float* centre1, const float* centre2, const int32_t* octave1,
                                              const float* scale, int nLevels, int capacity, int32_t* createdK, int32_t* createdI1,
                                              int32_t* createdI2, float* pos, float* normal, float* minDist, float* maxDist, uint8_t* descFrom,
                                              int32_t* nCreated, bool* over) {
  *over = false;
  if (!nCreated) return "NULL count";
  if (n1 < 0 || n1 > kTriHostMaxKeypoints) return "key frame 1 holds more than 16384 keypoints (or fewer than 0)";
  if (K < 0 || K > kTriHostMaxNeighbours) return "n_neighbours outside [0, 64]";
  if (capacity < 0) return "negative capacity";
  if (nLevels <= 0 || nLevels > ORBFE_MAX_LEVELS) return "n_levels outside (0, ORBFE_MAX_LEVELS]";
  if (!scale) return "NULL scale_factors";
  if (!centre1 || !tp_finite3(centre1)) return "key frame 1's centre is missing or not finite";
  if (kf1Id < 0) return "negative key-frame id";
  if (K > 0 && (!kf2Id || !centre2)) return "NULL array";
  if (K > 0 && n1 > 0 && (!match12 || !status || !x3d || !octave1)) return "NULL array";
  if (capacity > 0 && (!createdK || !createdI1 || !createdI2 || !pos || !normal || !minDist || !maxDist || !descFrom)) return "NULL output array";
  std::vector<uint8_t> seen;
  for (int k = 0; k < K; k++) {
    if (kf2Id[k] < 0) return "negative key-frame id";
    if (kf2Id[k] == kf1Id) return "two key frames have the same id";
    for (int j = 0; j < k; j++)
      if (kf2Id[j] == kf2Id[k]) return "two key frames have the same id";
    if (!tp_finite3(centre2 + 3 * (size_t)k)) return "a neighbour's centre is not finite";
    const int32_t* row = match12 + (size_t)k * n1;
    for (int i1 = 0; i1 < n1; i1++) {
      const int32_t i2 = row[i1];
      const uint8_t st = status[(size_t)k * n1 + i1];
      if (i2 < -1 || i2 >= kTriHostMaxKeypoints) return "match outside [-1, 16384)";
      if (st > ORBFE_TRI_SCALE) return "unknown status";
      if ((i2 < 0) != (st == ORBFE_TRI_NO_MATCH)) return "status and match12 disagree on which pairs exist";
      if (st == kTriCreated && (octave1[i1] < 0 || octave1[i1] >= nLevels)) return "octave of a created keypoint outside the level table";
    }
    if (tp_i2_twice(n1, row, kTriHostMaxKeypoints, &seen)) return "a keypoint of a neighbour is matched twice";
  }
  std::vector<int32_t> ks, i1s;
  const int count = tp_walk(n1, K, status, &ks, &i1s);
  *nCreated = count;
  if (count > capacity) {
    *over = true;
    return "more points are created than `capacity` (see *n_created)";
  }
  for (int w = 0; w < count; w++) {
    const int k = ks[(size_t)w], i1 = i1s[(size_t)w];
    const size_t at = (size_t)k * n1 + i1;
    const bool firstIs2 = kf2Id[k] < kf1Id;
    float* P = pos + 3 * (size_t)w;
    P[0] = x3d[3 * at]; P[1] = x3d[3 * at + 1]; P[2] = x3d[3 * at + 2];
    tp_normal_range(P, centre1, centre2 + 3 * (size_t)k, firstIs2, scale[octave1[i1]], scale[nLevels - 1], normal + 3 * (size_t)w, minDist + w,
                    maxDist + w);
    createdK[w] = k;
    createdI1[w] = i1;
    createdI2[w] = match12[at];
    descFrom[w] = firstIs2 ? 1 : 0;
  }
  return nullptr;
}

}  // namespace orbfe
