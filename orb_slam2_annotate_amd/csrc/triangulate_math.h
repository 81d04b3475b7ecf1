// triangulate_math.h -- the per-pair arithmetic of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:338-481), written
// once: k_triangulate.hip compiles it for the device, tests/cpp/triangulate_cpu.cpp for the host.  Plain C++ without a HIP
// include.  Arithmetic is binary64 on inputs widened from float (build with -ffp-contract=off); the reference computes in
// CV_32F with cv::SVD, so results agree with it to float rounding, not bit for bit.  Every index is a compile-time
// constant (after unrolling, in jacobi_math.h's 4 x 4 form) so that the 4 x 4 matrices stay in registers on the device.
#pragma once
#include <float.h>
#include <math.h>

#include "jacobi_math.h"  // jacobi_null4; ORBFE_HD

namespace orbfe {

// the statuses of include/orbfe.h (ORBFE_TRI_*), in the order the reference's `continue`s come
enum TriStatus {
  kTriNoMatch = 0, kTriCreated = 1, kTriLowParallax, kTriWZero, kTriBehind1, kTriBehind2, kTriReproj1, kTriReproj2,
  kTriDistZero, kTriScale
};

// a key frame as the loop reads it (orbfe_keyframe_camera without its arrays)
struct TriCamera {
  float Tcw[12];  // [Rcw | tcw] row-major 3 x 4
  float Ow[3];
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
};
// one keypoint of a pair
struct TriKeypoint {
  float x, y;        // mvKeysUn[i].pt
  float ur;          // mvuRight[i]
  float depth;       // mvDepth[i] (read only when ur >= 0)
  float xraw, yraw;  // mvKeys[i].pt (UnprojectStereo)
  float sigma2;      // mvLevelSigma2[octave]
  float scale;       // mvScaleFactors[octave]
};

// one matched pair of a call as it travels to the device: keypoint i1 of key frame 1 with keypoint i2 of neighbour k, and what
// the frames' own arrays do not hold
struct TriangulatePair {
  int k, i1, i2;
  float depth1, depth2;              // mvDepth (0 where the keypoint is monocular)
  float xraw1, yraw1, xraw2, yraw2;  // mvKeys[i].pt
};

// The right singular vector of the smallest singular value of the 4 x 4 `a` (row-major; destroyed): stands where the
// reference has vt.row(3) of cv::SVD::compute (:378-380); the sign is free and cancels in x / w.  The iteration is
// jacobi_math.h's; its sweep loop ends with the wave (JacobiWaveDone).
ORBFE_HD inline void tri_null_vector(double a[16], double x[4]) { jacobi_null4(a, x, JacobiWaveDone()); }

// KeyFrame::UnprojectStereo (src/KeyFrame.cc:658-674): reads the RAW keypoint position (mvKeys); Twc = [Rcw^T | Ow].  The
// callers hand in a depth > 0 (the host checks refuse others: the reference would return an empty matrix there)
ORBFE_HD inline void tri_unproject_stereo(const TriCamera& c, const TriKeypoint& k, double X[3]) {
  const double z = (double)k.depth;
  const double x = ((double)k.xraw - (double)c.cx) * z * (double)c.invfx;  // :665
  const double y = ((double)k.yraw - (double)c.cy) * z * (double)c.invfy;  // :666
  X[0] = (double)c.Tcw[0] * x + (double)c.Tcw[4] * y + (double)c.Tcw[8] * z + (double)c.Ow[0];  // :670
  X[1] = (double)c.Tcw[1] * x + (double)c.Tcw[5] * y + (double)c.Tcw[9] * z + (double)c.Ow[1];
  X[2] = (double)c.Tcw[2] * x + (double)c.Tcw[6] * y + (double)c.Tcw[10] * z + (double)c.Ow[2];
}

// the reprojection gate of one key frame (:411-436 / :438-462): `mbf` is KEY FRAME 1's for both (:429, :455 -- the second
// gate reads mpCurrentKeyFrame->mbf, not pKF2->mbf; kept)
ORBFE_HD inline bool tri_reprojection_fails(const TriCamera& c, const TriKeypoint& k, double mbf, double xc, double yc, double zc) {
  const double invz = 1.0 / zc;
  const double u = (double)c.fx * xc * invz + (double)c.cx, v = (double)c.fy * yc * invz + (double)c.cy;
  const double ex = u - (double)k.x, ey = v - (double)k.y;
  if (!(k.ur >= 0.0f)) return ex * ex + ey * ey > 5.991 * (double)k.sigma2;  // :423 / :449
  const double er = u - mbf * invz - (double)k.ur;
  return ex * ex + ey * ey + er * er > 7.8 * (double)k.sigma2;               // :434 / :460
}

// One matched pair (:338-481).  Returns the status; X is the new point when it is kTriCreated (written for every status
// past the three-way branch).  ratioFactor = 1.5f * mfScaleFactor (:278).
ORBFE_HD inline int tri_pair(const TriCamera& c1, const TriCamera& c2, const TriKeypoint& k1, const TriKeypoint& k2,
                             float ratioFactor, double X[3]) {
  const bool stereo1 = k1.ur >= 0.0f, stereo2 = k2.ur >= 0.0f;  // :340, :344
  // :347-348
  const double xn1x = ((double)k1.x - (double)c1.cx) * (double)c1.invfx, xn1y = ((double)k1.y - (double)c1.cy) * (double)c1.invfy;
  const double xn2x = ((double)k2.x - (double)c2.cx) * (double)c2.invfx, xn2y = ((double)k2.y - (double)c2.cy) * (double)c2.invfy;
  // ray = Rwc xn = Rcw^T xn (:350-351)
  const double r1x = (double)c1.Tcw[0] * xn1x + (double)c1.Tcw[4] * xn1y + (double)c1.Tcw[8];
  const double r1y = (double)c1.Tcw[1] * xn1x + (double)c1.Tcw[5] * xn1y + (double)c1.Tcw[9];
  const double r1z = (double)c1.Tcw[2] * xn1x + (double)c1.Tcw[6] * xn1y + (double)c1.Tcw[10];
  const double r2x = (double)c2.Tcw[0] * xn2x + (double)c2.Tcw[4] * xn2y + (double)c2.Tcw[8];
  const double r2y = (double)c2.Tcw[1] * xn2x + (double)c2.Tcw[5] * xn2y + (double)c2.Tcw[9];
  const double r2z = (double)c2.Tcw[2] * xn2x + (double)c2.Tcw[6] * xn2y + (double)c2.Tcw[10];
  const double cosRays = (r1x * r2x + r1y * r2y + r1z * r2z) /
                         (sqrt(r1x * r1x + r1y * r1y + r1z * r1z) * sqrt(r2x * r2x + r2y * r2y + r2z * r2z));  // :352
  double cosStereo1 = cosRays + 1.0, cosStereo2 = cosRays + 1.0;  // :354-356
  if (stereo1) cosStereo1 = cos(2.0 * atan2((double)c1.mb / 2.0, (double)k1.depth));       // :358-359
  else if (stereo2) cosStereo2 = cos(2.0 * atan2((double)c2.mb / 2.0, (double)k2.depth));  // :360-361 (`else if`)
  const double cosStereo = cosStereo1 < cosStereo2 ? cosStereo1 : cosStereo2;              // :363

  if (cosRays < cosStereo && cosRays > 0.0 && (stereo1 || stereo2 || cosRays < 0.9998)) {  // :368
    double a[16];  // :371-375
    a[0] = xn1x * (double)c1.Tcw[8] - (double)c1.Tcw[0]; a[1] = xn1x * (double)c1.Tcw[9] - (double)c1.Tcw[1];
    a[2] = xn1x * (double)c1.Tcw[10] - (double)c1.Tcw[2]; a[3] = xn1x * (double)c1.Tcw[11] - (double)c1.Tcw[3];
    a[4] = xn1y * (double)c1.Tcw[8] - (double)c1.Tcw[4]; a[5] = xn1y * (double)c1.Tcw[9] - (double)c1.Tcw[5];
    a[6] = xn1y * (double)c1.Tcw[10] - (double)c1.Tcw[6]; a[7] = xn1y * (double)c1.Tcw[11] - (double)c1.Tcw[7];
    a[8] = xn2x * (double)c2.Tcw[8] - (double)c2.Tcw[0]; a[9] = xn2x * (double)c2.Tcw[9] - (double)c2.Tcw[1];
    a[10] = xn2x * (double)c2.Tcw[10] - (double)c2.Tcw[2]; a[11] = xn2x * (double)c2.Tcw[11] - (double)c2.Tcw[3];
    a[12] = xn2y * (double)c2.Tcw[8] - (double)c2.Tcw[4]; a[13] = xn2y * (double)c2.Tcw[9] - (double)c2.Tcw[5];
    a[14] = xn2y * (double)c2.Tcw[10] - (double)c2.Tcw[6]; a[15] = xn2y * (double)c2.Tcw[11] - (double)c2.Tcw[7];
    double h[4];
    tri_null_vector(a, h);
    if (h[3] == 0.0) return kTriWZero;  // :382
    X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3];  // :386
  } else if (stereo1 && cosStereo1 < cosStereo2) {  // :389
    tri_unproject_stereo(c1, k1, X);
  } else if (stereo2 && cosStereo2 < cosStereo1) {  // :393
    tri_unproject_stereo(c2, k2, X);
  } else {
    return kTriLowParallax;  // :398
  }

  const double z1 = (double)c1.Tcw[8] * X[0] + (double)c1.Tcw[9] * X[1] + (double)c1.Tcw[10] * X[2] + (double)c1.Tcw[11];  // :403
  if (z1 <= 0.0) return kTriBehind1;  // :404
  const double z2 = (double)c2.Tcw[8] * X[0] + (double)c2.Tcw[9] * X[1] + (double)c2.Tcw[10] * X[2] + (double)c2.Tcw[11];  // :407
  if (z2 <= 0.0) return kTriBehind2;  // :408
  const double x1 = (double)c1.Tcw[0] * X[0] + (double)c1.Tcw[1] * X[1] + (double)c1.Tcw[2] * X[2] + (double)c1.Tcw[3];  // :413
  const double y1 = (double)c1.Tcw[4] * X[0] + (double)c1.Tcw[5] * X[1] + (double)c1.Tcw[6] * X[2] + (double)c1.Tcw[7];  // :414
  if (tri_reprojection_fails(c1, k1, (double)c1.mbf, x1, y1, z1)) return kTriReproj1;
  const double x2 = (double)c2.Tcw[0] * X[0] + (double)c2.Tcw[1] * X[1] + (double)c2.Tcw[2] * X[2] + (double)c2.Tcw[3];  // :440
  const double y2 = (double)c2.Tcw[4] * X[0] + (double)c2.Tcw[5] * X[1] + (double)c2.Tcw[6] * X[2] + (double)c2.Tcw[7];  // :441
  if (tri_reprojection_fails(c2, k2, (double)c1.mbf, x2, y2, z2)) return kTriReproj2;

  const double d1x = X[0] - (double)c1.Ow[0], d1y = X[1] - (double)c1.Ow[1], d1z = X[2] - (double)c1.Ow[2];  // :465-469
  const double d2x = X[0] - (double)c2.Ow[0], d2y = X[1] - (double)c2.Ow[1], d2z = X[2] - (double)c2.Ow[2];
  const double dist1 = sqrt(d1x * d1x + d1y * d1y + d1z * d1z), dist2 = sqrt(d2x * d2x + d2y * d2y + d2z * d2z);
  if (dist1 == 0.0 || dist2 == 0.0) return kTriDistZero;  // :471
  const double ratioDist = dist2 / dist1, ratioOctave = (double)k1.scale / (double)k2.scale;  // :474-475
  if (ratioDist * (double)ratioFactor < ratioOctave || ratioDist > ratioOctave * (double)ratioFactor) return kTriScale;  // :480
  return kTriCreated;
}

}  // namespace orbfe
