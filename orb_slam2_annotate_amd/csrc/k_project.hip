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
// reassociation, whatever flags the file is built with.
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
    const float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[0], X), __fmul_rn(c.Rcw[1], Y)), __fmul_rn(c.Rcw[2], Z)), c.tcw[0]);
    const float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[3], X), __fmul_rn(c.Rcw[4], Y)), __fmul_rn(c.Rcw[5], Z)), c.tcw[1]);
    const float zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[6], X), __fmul_rn(c.Rcw[7], Y)), __fmul_rn(c.Rcw[8], Z)), c.tcw[2]);
    if (zc < 0.0f) ok = false;
    // projection inside the image (:315-323)
    const float invz = __fdiv_rn(1.0f, zc);
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, xc), invz), c.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, yc), invz), c.cy);
    if (u < c.min_x || u > c.max_x) ok = false;
    if (v < c.min_y || v > c.max_y) ok = false;
    // distance inside the scale invariance region of the point (:325-332): cv::norm accumulates in double
    const float px = __fsub_rn(X, c.Ow[0]), py = __fsub_rn(Y, c.Ow[1]), pz = __fsub_rn(Z, c.Ow[2]);
    const double dpx = (double)px, dpy = (double)py, dpz = (double)pz;
    const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dpx, dpx), __dmul_rn(dpy, dpy)), __dmul_rn(dpz, dpz));
    const float dist = (float)__dsqrt_rn(d2);
    if (dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)) ok = false;
    // viewing angle (:334-340): Mat::dot accumulates in double
    const double dot = __dadd_rn(__dadd_rn(__dmul_rn(dpx, (double)r1.x), __dmul_rn(dpy, (double)r1.y)), __dmul_rn(dpz, (double)r1.z));
    const float viewCos = (float)__ddiv_rn(dot, (double)dist);
    if (viewCos < a.limit) ok = false;
    // MapPoint::PredictScale (:342-343)
    int lv = 0;
    if (ok) {
      const float ratio = __fdiv_rn(maxD, dist);
      const double cl = ceil(__ddiv_rn(log((double)ratio), (double)c.log_scale_factor));
      const int top = c.n_levels - 1;
      lv = cl > 0.0 ? (cl > (double)top ? top : (int)cl) : 0;  // (a NaN quotient -> 0)
    }
    const float xr = __fsub_rn(u, __fmul_rn(c.mbf, invz));
    if (a.inView) a.inView[i] = ok;
    if (a.level) a.level[i] = lv;
    if (a.viewCos) a.viewCos[i] = ok ? viewCos : 0.0f;
    if (a.projX) a.projX[i] = ok ? u : 0.0f;
    if (a.projY) a.projY[i] = ok ? v : 0.0f;
    if (a.projXr) a.projXr[i] = ok ? xr : 0.0f;
    if (a.invZ) a.invZ[i] = ok ? invz : 0.0f;
    if (a.dist) a.dist[i] = ok ? dist : 0.0f;
    if (a.qx) {
      // the windows of SearchByProjection(Frame&, vector<MapPoint*>&, th): RadiusByViewingCos (src/ORBmatcher.cc:140-146,
      // the compare in double), r *= th when th != 1.0 (:68-69), r * mvScaleFactors[level], levels [level - 1, level] (:71-73)
      float r = (double)(ok ? viewCos : 0.0f) > 0.998 ? 2.5f : 4.0f;
      if ((double)a.th != 1.0) r = __fmul_rn(r, a.th);
      a.qx[i] = ok ? u : 0.0f;
      a.qy[i] = ok ? v : 0.0f;
      a.qr[i] = __fmul_rn(r, a.scale[lv]);
      a.qmin[i] = lv - 1;
      a.qmax[i] = lv;
      a.qactive[i] = ok;
      a.qobs[i] = (fl & ORBFE_MP_OBSERVED) ? 1 : 0;
      if (a.qur) a.qur[i] = ok ? xr : 0.0f;
      if (a.inViewCopy) a.inViewCopy[i] = ok;
    }
  }
  if (a.qdesc) {  // (workgroup-uniform) the points' descriptors, gathered from the table: piece p = half (p & 1) of point base + p / 2
    const int cnt = a.n - base < kProjectThreads ? a.n - base : kProjectThreads;
    const uint4* src = reinterpret_cast<const uint4*>(a.table.desc);
    uint4* dst = reinterpret_cast<uint4*>(a.qdesc);
    for (int p = (int)threadIdx.x; p < 2 * cnt; p += kProjectThreads) {
      const int q = base + (p >> 1);
      dst[2 * (size_t)q + (p & 1)] = src[2 * (size_t)a.slot[q] + (p & 1)];
    }
  }
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
    const double nx = (double)r1.x, ny = (double)r1.y, nz = (double)r1.z;
    for (int k = 0; k < a.K; k++) {
      const orbfe_camera_pose& c = sPose[k];
      const size_t o = (size_t)k * a.n + i;
      bool ok = !(fl & ORBFE_MP_BAD) && !(a.skip && a.skip[o]) && !((inKf >> k) & 1);
      // 3D in camera coordinates (:969); the depth must be positive (:972)
      const float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[0], X), __fmul_rn(c.Rcw[1], Y)), __fmul_rn(c.Rcw[2], Z)), c.tcw[0]);
      const float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[3], X), __fmul_rn(c.Rcw[4], Y)), __fmul_rn(c.Rcw[5], Z)), c.tcw[1]);
      const float zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[6], X), __fmul_rn(c.Rcw[7], Y)), __fmul_rn(c.Rcw[8], Z)), c.tcw[2]);
      if (zc < 0.0f) ok = false;
      // normalised coordinates first (:975-980) -- not isInFrustum's (fx * xc) * invz
      const float invz = __fdiv_rn(1.0f, zc);
      const float x = __fmul_rn(xc, invz), y = __fmul_rn(yc, invz);
      const float u = __fadd_rn(__fmul_rn(c.fx, x), c.cx);
      const float v = __fadd_rn(__fmul_rn(c.fy, y), c.cy);
      // KeyFrame::IsInImage (src/KeyFrame.cc:653-656): the upper bounds are strict
      if (!(u >= c.min_x && u < c.max_x && v >= c.min_y && v < c.max_y)) ok = false;
      const float ur = __fsub_rn(u, __fmul_rn(c.mbf, invz));
      // distance inside the scale invariance region (:990-995): cv::norm accumulates in double
      const float px = __fsub_rn(X, c.Ow[0]), py = __fsub_rn(Y, c.Ow[1]), pz = __fsub_rn(Z, c.Ow[2]);
      const double dpx = (double)px, dpy = (double)py, dpz = (double)pz;
      const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dpx, dpx), __dmul_rn(dpy, dpy)), __dmul_rn(dpz, dpz));
      const float dist = (float)__dsqrt_rn(d2);
      if (dist < lo || dist > hi) ok = false;
      // viewing angle below 60 degrees (:1000): Mat::dot accumulates in double, the compare is in double, nothing is divided
      const double dot = __dadd_rn(__dadd_rn(__dmul_rn(dpx, nx), __dmul_rn(dpy, ny)), __dmul_rn(dpz, nz));
      if (dot < __dmul_rn(0.5, (double)dist)) ok = false;
      // MapPoint::PredictScale (:1003)
      int lv = 0;
      if (ok) {
        const float ratio = __fdiv_rn(maxD, dist);
        const double cl = ceil(__ddiv_rn(log((double)ratio), (double)c.log_scale_factor));
        const int top = c.n_levels - 1;
        lv = cl > 0.0 ? (cl > (double)top ? top : (int)cl) : 0;  // (a NaN quotient -> 0)
      }
      if (a.valid) a.valid[o] = ok;
      if (a.u) a.u[o] = ok ? u : 0.0f;
      if (a.v) a.v[o] = ok ? v : 0.0f;
      if (a.ur) a.ur[o] = ok ? ur : 0.0f;
      if (a.level) a.level[o] = lv;
      if (a.dist) a.dist[o] = ok ? dist : 0.0f;
      if (a.qx) {  // the windows of :1006-1028 as orbfe_fuse_search_multi builds them from the arrays above
        a.qx[o] = ok ? u : 0.0f;
        a.qy[o] = ok ? v : 0.0f;
        a.qr[o] = __fmul_rn(a.th, a.scale[lv]);
        a.qmin[o] = lv - 1;
        a.qmax[o] = lv;
        a.qactive[o] = ok;
        if (a.qur) a.qur[o] = ok ? ur : 0.0f;
        if (a.validCopy) a.validCopy[o] = ok;
      }
    }
  }
  if (a.qdesc) {  // (workgroup-uniform) the descriptors, gathered once for all K jobs: piece p = half (p & 1) of point base + p / 2
    const int cnt = a.n - base < kProjectThreads ? a.n - base : kProjectThreads;
    const uint4* src = reinterpret_cast<const uint4*>(a.table.desc);
    uint4* dst = reinterpret_cast<uint4*>(a.qdesc);
    for (int p = (int)threadIdx.x; p < 2 * cnt; p += kProjectThreads) {
      const int q = base + (p >> 1);
      dst[2 * (size_t)q + (p & 1)] = src[2 * (size_t)a.slot[q] + (p & 1)];
    }
  }
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
    const float xc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[0], X), __fmul_rn(c.Rcw[1], Y)), __fmul_rn(c.Rcw[2], Z)), c.tcw[0]);
    const float yc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[3], X), __fmul_rn(c.Rcw[4], Y)), __fmul_rn(c.Rcw[5], Z)), c.tcw[1]);
    const float zc = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rcw[6], X), __fmul_rn(c.Rcw[7], Y)), __fmul_rn(c.Rcw[8], Z)), c.tcw[2]);
    const float invz = __fdiv_rn(1.0f, zc);
    if (kForm == 0 && invz < 0.0f) ok = false;  // (:1524; the key-frame form has no depth test)
    const float u = __fadd_rn(__fmul_rn(__fmul_rn(c.fx, xc), invz), c.cx);
    const float v = __fadd_rn(__fmul_rn(__fmul_rn(c.fy, yc), invz), c.cy);
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
      // distance inside the scale invariance region of the point (:1682-1691): cv::norm accumulates in double
      const float px = __fsub_rn(X, c.Ow[0]), py = __fsub_rn(Y, c.Ow[1]), pz = __fsub_rn(Z, c.Ow[2]);
      const double dpx = (double)px, dpy = (double)py, dpz = (double)pz;
      const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dpx, dpx), __dmul_rn(dpy, dpy)), __dmul_rn(dpz, dpz));
      dist = (float)__dsqrt_rn(d2);
      if (dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)) ok = false;
      if (ok) {  // MapPoint::PredictScale (:1694)
        const float ratio = __fdiv_rn(maxD, dist);
        const double cl = ceil(__ddiv_rn(log((double)ratio), (double)c.log_scale_factor));
        const int top = c.n_levels - 1;
        lv = cl > 0.0 ? (cl > (double)top ? top : (int)cl) : 0;  // (a NaN quotient -> 0)
      }
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
    if (a.qx) {  // the windows as the host-array calls build them from the arrays above
      a.qx[o] = ok ? u : 0.0f;
      a.qy[o] = ok ? v : 0.0f;
      a.qr[o] = r;
      a.qmin[o] = lo;
      a.qmax[o] = hi;
      a.qactive[o] = ok;
      if (kForm == 0) {
        a.qobs[o] = (fl & ORBFE_MP_OBSERVED) ? 1 : 0;
        if (a.qur) a.qur[o] = ok ? ur : 0.0f;
      }
      if (a.validCopy) a.validCopy[o] = ok;
    }
  }
  if (a.qdesc) {  // (workgroup-uniform) the points' descriptors: piece p = half (p & 1) of point off + base + p / 2
    const int cnt = nk - base < kProjectThreads ? nk - base : kProjectThreads;
    const uint4* src = reinterpret_cast<const uint4*>(a.table.desc);
    uint4* dst = reinterpret_cast<uint4*>(a.qdesc);
    for (int p = (int)threadIdx.x; p < 2 * cnt; p += kProjectThreads) {
      const size_t q = (size_t)off + base + (p >> 1);
      dst[2 * q + (p & 1)] = src[2 * (size_t)a.slot[q] + (p & 1)];
    }
  }
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
    const float X = r0.x, Y = r0.y, Z = r0.z, minD = r0.w, maxD = r1.w;
    // source camera (:1309), then target camera (:1310)
    const float x1 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rw[0], X), __fmul_rn(c.Rw[1], Y)), __fmul_rn(c.Rw[2], Z)), c.tw[0]);
    const float y1 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rw[3], X), __fmul_rn(c.Rw[4], Y)), __fmul_rn(c.Rw[5], Z)), c.tw[1]);
    const float z1 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.Rw[6], X), __fmul_rn(c.Rw[7], Y)), __fmul_rn(c.Rw[8], Z)), c.tw[2]);
    const float x2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.sR[0], x1), __fmul_rn(c.sR[1], y1)), __fmul_rn(c.sR[2], z1)), c.t[0]);
    const float y2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.sR[3], x1), __fmul_rn(c.sR[4], y1)), __fmul_rn(c.sR[5], z1)), c.t[1]);
    const float z2 = __fadd_rn(__fadd_rn(__fadd_rn(__fmul_rn(c.sR[6], x1), __fmul_rn(c.sR[7], y1)), __fmul_rn(c.sR[8], z1)), c.t[2]);
    if (z2 < 0.0f) ok = false;  // (:1313)
    const float invz = __fdiv_rn(1.0f, z2);
    const float x = __fmul_rn(x2, invz), y = __fmul_rn(y2, invz);
    const float u = __fadd_rn(__fmul_rn(c.fx, x), c.cx);
    const float v = __fadd_rn(__fmul_rn(c.fy, y), c.cy);
    // KeyFrame::IsInImage (src/KeyFrame.cc:653-656): the upper bounds are strict; a NaN coordinate is rejected here
    if (!(u >= c.min_x && u < c.max_x && v >= c.min_y && v < c.max_y)) ok = false;
    // cv::norm(p3Dc2) (:1330) accumulates in double: the camera-frame vector, not P - Ow
    const double dx = (double)x2, dy = (double)y2, dz = (double)z2;
    const double d2 = __dadd_rn(__dadd_rn(__dmul_rn(dx, dx), __dmul_rn(dy, dy)), __dmul_rn(dz, dz));
    const float dist = (float)__dsqrt_rn(d2);
    if (dist < __fmul_rn(0.8f, minD) || dist > __fmul_rn(1.2f, maxD)) ok = false;
    int lv = 0;
    if (ok) {  // MapPoint::PredictScale (:1337)
      const float ratio = __fdiv_rn(maxD, dist);
      const double cl = ceil(__ddiv_rn(log((double)ratio), (double)c.log_scale_factor));
      const int top = c.n_levels - 1;
      lv = cl > 0.0 ? (cl > (double)top ? top : (int)cl) : 0;  // (a NaN quotient -> 0)
    }
    if (a.valid) a.valid[o] = ok;
    if (a.u) a.u[o] = ok ? u : 0.0f;
    if (a.v) a.v[o] = ok ? v : 0.0f;
    if (a.level) a.level[o] = lv;
    if (a.dist) a.dist[o] = ok ? dist : 0.0f;
    if (a.qx) {  // the windows of :1340-1359 as orbfe_search_by_sim3 builds them from the arrays above
      const float* scale = a.scale + ((sp.flags & 2) ? a.nLevels : 0);
      a.qx[o] = ok ? u : 0.0f;
      a.qy[o] = ok ? v : 0.0f;
      a.qr[o] = __fmul_rn(a.th, scale[lv]);
      a.qmin[o] = lv - 1;
      a.qmax[o] = lv;
      a.qactive[o] = ok;
    }
  }
  if (a.qdesc && (sp.flags & 1)) {  // (workgroup-uniform) the leg's descriptors; a point without a slot gets zeros, nothing reads them
    const int cnt = sp.n - base < kProjectThreads ? sp.n - base : kProjectThreads;
    const uint4* src = reinterpret_cast<const uint4*>(a.table.desc);
    uint4* dst = reinterpret_cast<uint4*>(a.qdesc);
    for (int p = (int)threadIdx.x; p < 2 * cnt; p += kProjectThreads) {
      const size_t q = (size_t)sp.slotOff + base + (p >> 1);
      const int s = a.slot[q];
      dst[2 * q + (p & 1)] = s >= 0 ? src[2 * (size_t)s + (p & 1)] : make_uint4(0u, 0u, 0u, 0u);
    }
  }
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
