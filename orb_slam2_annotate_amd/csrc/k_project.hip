// k_project.hip -- the pose arithmetic in front of Tracking::SearchLocalPoints on the device-resident map points:
// Frame::isInFrustum (src/Frame.cc:292-353) with MapPoint::PredictScale, the prologue of ORBmatcher::Fuse for K key frames
// (k_project_fuse), the prologues of the last-frame and key-frame SearchByProjection (k_project_track), the prologue of
// SearchBySim3 for many legs (k_project_sim3), and the scatter that keeps the table up to date.
// The kernels are bandwidth-trivial (64 bytes of table per point, a few thousand points): one lane per point, the table
// records as 16-byte loads, the descriptor rows moved by the whole workgroup as 16-byte pieces.
#include <hip/hip_runtime.h>

#include "kernels.h"
#include "match_kernels.h"
#include "obsgraph_host.h"

namespace orbfe {

namespace {

constexpr int kProjectThreads = 256;

// Every operation is written with the round-to-nearest intrinsics, in the order include/orbfe.h states: no contraction, no
// reassociation, whatever flags the file is built with.  The steps the prologues share stand here once; they inline.

struct Vec3 { float x, y, z; };
// R (3 x 3, row-major) * (X, Y, Z) + t: a point into a camera's coordinates
__device__ __forceinline__ Vec3 transform(const float* R, const float* t, float X, float Y, float Z) {
  Vec3 p;
  p.x = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[0], X), __fmul_rn(R[1], Y)), __fmul_rn(R[2], Z)), t[0]);
  p.y = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[3], X), __fmul_rn(R[4], Y)), __fmul_rn(R[5], Z)), t[1]);
  p.z = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(R[6], X), __fmul_rn(R[7], Y)), __fmul_rn(R[8], Z)), t[2]);
  return p;
}
// cv::norm and Mat::dot of three floats accumulate in double
__device__ __forceinline__ double dot3(Vec3 a, float bx, float by, float bz) {
  return __dadd_rn(__dadd_rn(__dmul_rn((double)a.x, (double)bx), __dmul_rn((double)a.y, (double)by)), __dmul_rn((double)a.z, (double)bz));
}
__device__ __forceinline__ float norm3(Vec3 a) { return (float)__dsqrt_rn(dot3(a, a.x, a.y, a.z)); }
// MapPoint::PredictScale: ceil(log(maxD / dist) / log_scale_factor), clamped to the pyramid; a NaN quotient -> 0
__device__ __forceinline__ int predict_scale(float maxD, float dist, float logScaleFactor, int nLevels) {
  const float ratio = __fdiv_rn(maxD, dist);
  const double cl = ceil(__ddiv_rn(log((double)ratio), (double)logScaleFactor));
  const int top = nLevels - 1;
  return cl > 0.0 ? (cl > (double)top ? top : (int)cl) : 0;
}
// the window of point o as the host-array searches build it: centre (u, v) or 0 when rejected, radius r, octaves [lo, hi],
// and the optional arrays (match_kernels.h: QueryOut) the call asked for
__device__ __forceinline__ void store_window(const QueryOut& q, size_t o, bool ok, float u, float v, float r, int lo, int hi, float ur,
                                             uint8_t fl) {
  q.x[o] = ok ? u : 0.0f;
  q.y[o] = ok ? v : 0.0f;
  q.r[o] = r;
  q.minLevel[o] = lo;
  q.maxLevel[o] = hi;
  q.active[o] = ok;
  if (q.obs) q.obs[o] = (fl & ORBFE_MP_OBSERVED) ? 1 : 0;
  if (q.ur) q.ur[o] = ok ? ur : 0.0f;
  if (q.validCopy) q.validCopy[o] = ok;
}
// (workgroup-uniform) the descriptors of the workgroup's points -- positions off + base .. of slot[], n points in the list --
// gathered from the table into out[] at the same positions: piece p = half (p & 1) of point off + base + p / 2.  sparse
// (k_project_sim3): slot -1 is "no map point" and gets zeros, nothing reads them
__device__ __forceinline__ void gather_desc(const MapPointsDevice& t, const int32_t* slot, uint8_t* out, size_t off, int n, int base,
                                            bool sparse) {
  const int cnt = n - base < kProjectThreads ? n - base : kProjectThreads;
  const uint4* src = reinterpret_cast<const uint4*>(t.desc);
  uint4* dst = reinterpret_cast<uint4*>(out);
  for (int p = (int)threadIdx.x; p < 2 * cnt; p += kProjectThreads) {
    const size_t q = off + base + (p >> 1);
    const int s = slot[q];
    dst[2 * q + (p & 1)] = sparse && s < 0 ? make_uint4(0u, 0u, 0u, 0u) : src[2 * (size_t)s + (p & 1)];
  }
}

__global__ __launch_bounds__(kProjectThreads) void k_project_frustum(const ProjectArgs a) {
  const int base = blockIdx.x * kProjectThreads;
  const int i = base + (int)threadIdx.x;
  if (i < a.n) {
    const int s = a.slot[i];
    const float4 r0 = a.table.rec[2 * (size_t)s], r1 = a.table.rec[2 * (size_t)s + 1];
    const uint8_t fl = a.table.flags[s];
    const orbfe_camera_pose& c = a.cam;
    const float X = r0.x, Y = r0.y, Z = r0.z, minD = r0.w, maxD = r1.w;
    bool ok = !(fl & ORBFE_MP_BAD) && !(a.skip && a.skip[i]);
    // 3D in camera coordinates (:305-309); the depth must be positive (:311-313)
    const Vec3 pc = transform(c.Rcw, c.tcw, X, Y, Z);
    if (pc.z < 0.0f) ok = false;
    // projection inside the image (:315-323)
    const float invz = __fdiv_rn(1.0f, pc.z);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, pc.x), invz), c.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, pc.y), invz), c.cy);
    if (u < c.min_x || u > c.max_x) ok = false;
    if (v < c.min_y || v > c.max_y) ok = false;
    // distance inside the scale invariance region of the point (:325-332)
    const Vec3 po = {__fsub_rn(X, c.Ow[0]), __fsub_rn(Y, c.Ow[1]), __fsub_rn(Z, c.Ow[2])};
    const float dist = norm3(po);
    if (dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)) ok = false;
    // viewing angle (:334-340)
    const float viewCos = (float)__ddiv_rn(dot3(po, r1.x, r1.y, r1.z), (double)dist);
    if (viewCos < a.limit) ok = false;
    int lv = 0;
    if (ok) lv = predict_scale(maxD, dist, c.log_scale_factor, c.n_levels);  // (:342-343)
    const float xr = __fsub_rn(u, __fmul_rn(c.mbf, invz));
    if (a.inView) a.inView[i] = ok;
    if (a.level) a.level[i] = lv;
    if (a.viewCos) a.viewCos[i] = ok ? viewCos : 0.0f;
    if (a.projX) a.projX[i] = ok ? u : 0.0f;
    if (a.projY) a.projY[i] = ok ? v : 0.0f;
    if (a.projXr) a.projXr[i] = ok ? xr : 0.0f;
    if (a.invZ) a.invZ[i] = ok ? invz : 0.0f;
    if (a.dist) a.dist[i] = ok ? dist : 0.0f;
    if (a.q.x) {
      // the windows of SearchByProjection(Frame&, vector<MapPoint*>&, th): RadiusByViewingCos (src/ORBmatcher.cc:140-146,
      // the compare in double), r *= th when th != 1.0 (:68-69), r * mvScaleFactors[level], levels [level - 1, level] (:71-73)
      float r = (double)(ok ? viewCos : 0.0f) > 0.998 ? 2.5f : 4.0f;
      if ((double)a.th != 1.0) r = __fmul_rn(r, a.th);
      store_window(a.q, (size_t)i, ok, u, v, __fmul_rn(r, a.scale[lv]), lv - 1, lv, xr, fl);
    }
  }
  if (a.q.desc) gather_desc(a.table, a.slot, a.q.desc, 0, a.n, base, false);
}

// The prologue of ORBmatcher::Fuse (src/ORBmatcher.cc:960-1006) for 256 consecutive points x K key-frame poses: the two table
// records and the flag byte of a point are read once, the poses and kf slots wait in LDS (K x 104 bytes), and every result array
// is [k * n + i], so that a wave's stores of one k are consecutive.  The arithmetic is include/orbfe.h's (orbfe_project_fuse),
// operation by operation.  The Sim3 overload (:1135-1184) computes 1.0 / z in double and rounds the quotient to float: that
// is the float division below, since a double quotient of two floats rounded to float is correctly rounded (53 >= 2 * 24 + 2).
__global__ __launch_bounds__(kProjectThreads) void k_project_fuse(const FuseArgs a) {
  __shared__ orbfe_camera_pose sPose[kFuseMaxKeyFrames];
  __shared__ int32_t sKf[kFuseMaxKeyFrames];
  {
    constexpr int kWords = (int)(sizeof(orbfe_camera_pose) / 4);
    const uint32_t* src = reinterpret_cast<const uint32_t*>(a.pose);
    uint32_t* dst = reinterpret_cast<uint32_t*>(sPose);
    for (int w = (int)threadIdx.x; w < a.K * kWords; w += kProjectThreads) dst[w] = src[w];
    if ((int)threadIdx.x < a.K) sKf[threadIdx.x] = a.rows ? a.kfSlot[threadIdx.x] : -1;
  }
  __syncthreads();
  const int base = blockIdx.x * kProjectThreads;
  const int i = base + (int)threadIdx.x;
  if (i < a.n) {
    const int s = a.slot[i];
    const float4 r0 = a.table.rec[2 * (size_t)s], r1 = a.table.rec[2 * (size_t)s + 1];
    const uint8_t fl = a.table.flags[s];
    const float X = r0.x, Y = r0.y, Z = r0.z, minD = r0.w, maxD = r1.w;
    // MapPoint::IsInKeyFrame (:965) for all K key frames from one walk over the row: bit k = the row names kfSlot[k]
    unsigned long long inKf = 0;
    if (a.rows && s < a.pointCap) {
      int cnt = a.meta[s].count;
      cnt = cnt < a.rowWidth ? cnt : a.rowWidth;
      const ObsEntry* row = a.rows + (size_t)s * a.rowWidth;
      for (int e = 0; e < cnt; e++) {
        const int32_t kf = row[e].kf;
        for (int k = 0; k < a.K; k++)
          if (sKf[k] == kf) inKf |= 1ull << k;
      }
    }
    const float lo = __fmul_rn(0.8f, minD), hi = __fmul_rn(1.2f, maxD);
    for (int k = 0; k < a.K; k++) {
      const orbfe_camera_pose& c = sPose[k];
      const size_t o = (size_t)k * a.n + i;
      bool ok = !(fl & ORBFE_MP_BAD) && !(a.skip && a.skip[o]) && !((inKf >> k) & 1);
      // 3D in camera coordinates (:969); the depth must be positive (:972)
      const Vec3 pc = transform(c.Rcw, c.tcw, X, Y, Z);
      if (pc.z < 0.0f) ok = false;
      // normalised coordinates first (:975-980) -- not isInFrustum's (fx * xc) * invz
      const float invz = __fdiv_rn(1.0f, pc.z);
      const float x = __fmul_rn(pc.x, invz), y = __fmul_rn(pc.y, invz);
      const float u = __fadd_rn(__fmul_rn(c.fx, x), c.cx);
      const float v = __fadd_rn(__fmul_rn(c.fy, y), c.cy);
      // KeyFrame::IsInImage (src/KeyFrame.cc:653-656): the upper bounds are strict
      if (!(u >= c.min_x && u < c.max_x && v >= c.min_y && v < c.max_y)) ok = false;
      const float ur = __fsub_rn(u, __fmul_rn(c.mbf, invz));
      // distance inside the scale invariance region (:990-995)
      const Vec3 po = {__fsub_rn(X, c.Ow[0]), __fsub_rn(Y, c.Ow[1]), __fsub_rn(Z, c.Ow[2])};
      const float dist = norm3(po);
      if (dist < lo || dist > hi) ok = false;
      // viewing angle below 60 degrees (:1000): the compare is in double, nothing is divided
      if (dot3(po, r1.x, r1.y, r1.z) < __dmul_rn(0.5, (double)dist)) ok = false;
      int lv = 0;
      if (ok) lv = predict_scale(maxD, dist, c.log_scale_factor, c.n_levels);  // (:1003)
      if (a.valid) a.valid[o] = ok;
      if (a.u) a.u[o] = ok ? u : 0.0f;
      if (a.v) a.v[o] = ok ? v : 0.0f;
      if (a.ur) a.ur[o] = ok ? ur : 0.0f;
      if (a.level) a.level[o] = lv;
      if (a.dist) a.dist[o] = ok ? dist : 0.0f;
      // the windows of :1006-1028 as orbfe_fuse_search_multi builds them from the arrays above
      if (a.q.x) store_window(a.q, o, ok, u, v, __fmul_rn(a.th, a.scale[lv]), lv - 1, lv, ur, fl);
    }
  }
  if (a.q.desc) gather_desc(a.table, a.slot, a.q.desc, 0, a.n, base, false);  // once for all K jobs
}

// The prologues of SearchByProjection(CurrentFrame, LastFrame, th, bMono) (kForm 0, src/ORBmatcher.cc:1516-1550) and of
// SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (kForm 1, :1665-1699) for K jobs over concatenated lists:
// blockIdx.y is the job, a workgroup owns 256 consecutive points of it, and a job shorter than the longest leaves its spare
// workgroups at once.  The pose and th of the job are uniform reads.  The arithmetic is include/orbfe.h's
// (orbfe_project_last_frame / orbfe_project_keyframe), operation by operation.  The reference's 1.0 / z in double, rounded to
// float, is the float division below: a double quotient of two floats rounded to float is correctly rounded (53 >= 2 * 24 + 2).
template <int kForm>
__global__ __launch_bounds__(kProjectThreads) void k_project_track(const TrackArgs a) {
  const int k = (int)blockIdx.y;
  const int off = a.offsets[k], nk = a.offsets[k + 1] - off;
  const int base = blockIdx.x * kProjectThreads;
  if (base >= nk) return;  // (workgroup-uniform)
  const int i = base + (int)threadIdx.x;
  if (i < nk) {
    const size_t o = (size_t)off + i;
    const int s = a.slot[o];
    const float4 r0 = a.table.rec[2 * (size_t)s], r1 = a.table.rec[2 * (size_t)s + 1];
    const uint8_t fl = a.table.flags[s];
    const orbfe_camera_pose& c = a.pose[k];
    const float th = a.th ? a.th[k] : 0.0f;
    const float X = r0.x, Y = r0.y, Z = r0.z, minD = r0.w, maxD = r1.w;
    // pMP && !mvbOutlier[i] is the caller's list (:1510-1514: isBad is NOT asked); !isBad() && !sAlreadyFound.count(pMP) (:1663)
    bool ok = !(a.skip && a.skip[o]);
    if (kForm == 1 && (fl & ORBFE_MP_BAD)) ok = false;
    const Vec3 pc = transform(c.Rcw, c.tcw, X, Y, Z);
    const float invz = __fdiv_rn(1.0f, pc.z);
    if (kForm == 0 && invz < 0.0f) ok = false;  // (:1524; the key-frame form has no depth test)
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, pc.x), invz), c.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, pc.y), invz), c.cy);
    // inside the image, bounds included (:1533-1536, :1676-1679); a NaN coordinate is rejected here
    if (!(u >= c.min_x && u <= c.max_x && v >= c.min_y && v <= c.max_y)) ok = false;
    int lv = 0, lo = 0, hi = 0;
    float dist = 0.0f;
    const float ur = __fsub_rn(u, __fmul_rn(c.mbf, invz));
    if (kForm == 0) {
      lv = ok ? a.lastOctave[o] : 0;
      if (a.mode == 1) { lo = lv; hi = -1; }       // bForward:  GetFeaturesInArea(u, v, radius, nLastOctave)
      else if (a.mode == 2) { lo = 0; hi = lv; }   // bBackward: (u, v, radius, 0, nLastOctave)
      else { lo = lv - 1; hi = lv + 1; }
    } else {
      // distance inside the scale invariance region of the point (:1682-1691)
      const Vec3 po = {__fsub_rn(X, c.Ow[0]), __fsub_rn(Y, c.Ow[1]), __fsub_rn(Z, c.Ow[2])};
      dist = norm3(po);
      if (dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)) ok = false;
      if (ok) lv = predict_scale(maxD, dist, c.log_scale_factor, c.n_levels);  // (:1694)
      lo = lv - 1; hi = lv + 1;
    }
    const float r = a.scale ? __fmul_rn(th, a.scale[lv]) : 0.0f;  // (:1541, :1697)
    if (a.valid) a.valid[o] = ok;
    if (a.u) a.u[o] = ok ? u : 0.0f;
    if (a.v) a.v[o] = ok ? v : 0.0f;
    if (a.invZ) a.invZ[o] = ok ? invz : 0.0f;
    if (kForm == 0) {
      if (a.ur) a.ur[o] = ok ? ur : 0.0f;
      if (a.radius) a.radius[o] = ok ? r : 0.0f;
    } else {
      if (a.level) a.level[o] = lv;
      if (a.dist) a.dist[o] = ok ? dist : 0.0f;
    }
    // the windows as the host-array calls build them from the arrays above (q.obs and q.ur: the last-frame form alone)
    if (a.q.x) store_window(a.q, o, ok, u, v, r, lo, hi, ur, fl);
  }
  if (a.q.desc) gather_desc(a.table, a.slot, a.q.desc, (size_t)off, nk, base, false);
}

// The prologue of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1298-1340, :1379-1420) for many legs: blockIdx.y is the leg (one
// direction of one candidate), a workgroup owns 256 consecutive points of it, and a leg shorter than the longest leaves its
// spare workgroups at once.  The leg record and its span are uniform reads.  The arithmetic is include/orbfe.h's
// (orbfe_project_sim3), operation by operation.  The reference's 1.0 / z in double, rounded to float, is the float division
// below: a double quotient of two floats rounded to float is correctly rounded (53 >= 2 * 24 + 2).
__global__ __launch_bounds__(kProjectThreads) void k_project_sim3(const Sim3Args a) {
  const Sim3Span sp = a.span[blockIdx.y];
  const int base = blockIdx.x * kProjectThreads;
  if (base >= sp.n) return;  // (workgroup-uniform)
  const int i = base + (int)threadIdx.x;
  if (i < sp.n) {
    const orbfe_sim3_leg& c = a.leg[blockIdx.y];
    const size_t o = (size_t)sp.outOff + i;
    const int s = a.slot[(size_t)sp.slotOff + i];
    // pMP && !vbAlreadyMatched[i] && !pMP->isBad() (:1300-1306): slot -1 is "no map point" and reads nothing of the table
    float4 r0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), r1 = r0;
    uint8_t fl = ORBFE_MP_BAD;
    if (s >= 0) { r0 = a.table.rec[2 * (size_t)s]; r1 = a.table.rec[2 * (size_t)s + 1]; fl = a.table.flags[s]; }
    bool ok = s >= 0 && !(a.skip && a.skip[o]) && !(fl & ORBFE_MP_BAD);
    const float minD = r0.w, maxD = r1.w;
    // source camera (:1309), then target camera (:1310)
    const Vec3 p1 = transform(c.Rw, c.tw, r0.x, r0.y, r0.z);
    const Vec3 p2 = transform(c.sR, c.t, p1.x, p1.y, p1.z);
    if (p2.z < 0.0f) ok = false;  // (:1313)
    const float invz = __fdiv_rn(1.0f, p2.z);
    const float x = __fmul_rn(p2.x, invz), y = __fmul_rn(p2.y, invz);
    const float u = __fadd_rn(__fmul_rn(c.fx, x), c.cx);
    const float v = __fadd_rn(__fmul_rn(c.fy, y), c.cy);
    // KeyFrame::IsInImage (src/KeyFrame.cc:653-656): the upper bounds are strict; a NaN coordinate is rejected here
    if (!(u >= c.min_x && u < c.max_x && v >= c.min_y && v < c.max_y)) ok = false;
    const float dist = norm3(p2);  // cv::norm(p3Dc2) (:1330): the camera-frame vector, not P - Ow
    if (dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)) ok = false;
    int lv = 0;
    if (ok) lv = predict_scale(maxD, dist, c.log_scale_factor, c.n_levels);  // (:1337)
    if (a.valid) a.valid[o] = ok;
    if (a.u) a.u[o] = ok ? u : 0.0f;
    if (a.v) a.v[o] = ok ? v : 0.0f;
    if (a.level) a.level[o] = lv;
    if (a.dist) a.dist[o] = ok ? dist : 0.0f;
    if (a.q.x) {  // the windows of :1340-1359 as orbfe_search_by_sim3 builds them from the arrays above
      const float* scale = a.scale + ((sp.flags & 2) ? a.nLevels : 0);
      store_window(a.q, o, ok, u, v, __fmul_rn(a.th, scale[lv]), lv - 1, lv, 0.0f, fl);
    }
  }
  // the leg's descriptors lie where its slots do, so the K legs that read one list share one gather (flags & 1)
  if (a.q.desc && (sp.flags & 1)) gather_desc(a.table, a.slot, a.q.desc, (size_t)sp.slotOff, sp.n, base, true);
}

// vbAlreadyMatched2 (:1282-1292) from the observation rows: one lane per (candidate, keypoint of KF1)
__global__ __launch_bounds__(kProjectThreads) void k_sim3_already(const ObsEntry* __restrict__ rows, const ObsPointMeta* __restrict__ meta,
                                                                  int rowWidth, int pointCap, int n1, const int32_t* __restrict__ matched,
                                                                  const int32_t* __restrict__ kfSlot, const int32_t* __restrict__ offsets2,
                                                                  uint8_t* __restrict__ already2) {
  const int k = (int)blockIdx.y;
  const int i = blockIdx.x * kProjectThreads + (int)threadIdx.x;
  if (i >= n1) return;
  const int s = matched[(size_t)k * n1 + i];
  if (s < 0 || s >= pointCap) return;
  const int off = offsets2[k], n2 = offsets2[k + 1] - off, kf = kfSlot[k];
  int cnt = meta[s].count;
  cnt = cnt < rowWidth ? cnt : rowWidth;
  const ObsEntry* row = rows + (size_t)s * rowWidth;
  for (int e = 0; e < cnt; e++)
    if (row[e].kf == kf) {
      const int idx = (int)row[e].idx;
      if (idx < n2) already2[(size_t)off + idx] = 1;
    }
}

__global__ __launch_bounds__(kProjectThreads) void k_mappoints_scatter(const MapPointsDevice t, int n, const int32_t* __restrict__ slot,
                                                                       const float4* __restrict__ rec, const uint8_t* __restrict__ flags,
                                                                       const uint8_t* __restrict__ desc) {
  const int base = blockIdx.x * kProjectThreads;
  const int i = base + (int)threadIdx.x;
  if (i < n) {
    const int s = slot[i];
    t.rec[2 * (size_t)s] = rec[2 * (size_t)i];
    t.rec[2 * (size_t)s + 1] = rec[2 * (size_t)i + 1];
    t.flags[s] = flags[i];
  }
  if (desc) {  // (uniform)
    const int cnt = n - base < kProjectThreads ? n - base : kProjectThreads;
    const uint4* src = reinterpret_cast<const uint4*>(desc);
    uint4* dst = reinterpret_cast<uint4*>(t.desc);
    for (int p = (int)threadIdx.x; p < 2 * cnt; p += kProjectThreads) {
      const int q = base + (p >> 1);
      dst[2 * (size_t)slot[q] + (p & 1)] = src[2 * (size_t)q + (p & 1)];
    }
  }
}

// the descriptors of slot[0 .. n), moved by the whole workgroup as 16-byte pieces: piece p = half (p & 1) of point p / 2
__global__ __launch_bounds__(kProjectThreads) void k_mappoints_read_descriptors(const MapPointsDevice t, int n, const int32_t* __restrict__ slot,
                                                                                uint8_t* __restrict__ desc) {
  const size_t p = (size_t)blockIdx.x * kProjectThreads + threadIdx.x;
  if (p >= 2 * (size_t)n) return;
  reinterpret_cast<uint4*>(desc)[p] = reinterpret_cast<const uint4*>(t.desc)[2 * (size_t)slot[p >> 1] + (p & 1)];
}

}  // namespace

void launch_project_frustum(hipStream_t s, const ProjectArgs& a) {
  if (a.n <= 0) return;
  hipLaunchKernelGGL(k_project_frustum, dim3((a.n + kProjectThreads - 1) / kProjectThreads), dim3(kProjectThreads), 0, s, a);
}

void launch_project_fuse(hipStream_t s, const FuseArgs& a) {
  if (a.n <= 0 || a.K <= 0 || a.K > kFuseMaxKeyFrames) return;
  hipLaunchKernelGGL(k_project_fuse, dim3((a.n + kProjectThreads - 1) / kProjectThreads), dim3(kProjectThreads), 0, s, a);
}

void launch_project_track(hipStream_t s, const TrackArgs& a, int maxN) {
  if (maxN <= 0 || a.K <= 0 || a.K > kTrackMaxJobs) return;
  const dim3 grid((maxN + kProjectThreads - 1) / kProjectThreads, a.K);
  if (a.form == 0) hipLaunchKernelGGL(k_project_track<0>, grid, dim3(kProjectThreads), 0, s, a);
  else hipLaunchKernelGGL(k_project_track<1>, grid, dim3(kProjectThreads), 0, s, a);
}

void launch_project_sim3(hipStream_t s, const Sim3Args& a, int maxN) {
  if (maxN <= 0 || a.nLegs <= 0 || a.nLegs > kSim3MaxLegs) return;
  hipLaunchKernelGGL(k_project_sim3, dim3((maxN + kProjectThreads - 1) / kProjectThreads, a.nLegs), dim3(kProjectThreads), 0, s, a);
}

void launch_sim3_already(hipStream_t s, const ObsEntry* rows, const ObsPointMeta* meta, int rowWidth, int pointCap, int K, int n1,
                         const int32_t* matched, const int32_t* kfSlot, const int32_t* offsets2, uint8_t* already2) {
  if (K <= 0 || n1 <= 0) return;
  hipLaunchKernelGGL(k_sim3_already, dim3((n1 + kProjectThreads - 1) / kProjectThreads, K), dim3(kProjectThreads), 0, s, rows, meta, rowWidth,
                     pointCap, n1, matched, kfSlot, offsets2, already2);
}

void launch_mappoints_scatter(hipStream_t s, const MapPointsDevice& t, int n, const int32_t* slot, const float4* rec,
                              const uint8_t* flags, const uint8_t* desc) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_mappoints_scatter, dim3((n + kProjectThreads - 1) / kProjectThreads), dim3(kProjectThreads), 0, s, t, n, slot, rec,
                     flags, desc);
}

void launch_mappoints_read_descriptors(hipStream_t s, const MapPointsDevice& t, int n, const int32_t* slot, uint8_t* desc) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_mappoints_read_descriptors, dim3((unsigned)((2 * (size_t)n + kProjectThreads - 1) / kProjectThreads)),
                     dim3(kProjectThreads), 0, s, t, n, slot, desc);
}

}  // namespace orbfe
