// initializer_reconstruct_math.h -- what Initializer::Initialize does after the choice of the model (src/Initializer.cc): the
// motion hypotheses of ReconstructH (:667-775, 8 of them, Faugeras) and of ReconstructF / DecomposeE (:546-566, :1034-1057, 4),
// and CheckRT (:913-1029) of one hypothesis over the inlier pairs, written once: k_init_reconstruct.hip compiles it for the
// device, tests/cpp/initializer_reconstruct_cpu.cpp and tests/cpp/initializer_reconstruct_host_san.cpp for the host.  Plain
// C++ without a HIP include.  Arithmetic is binary64 on inputs widened from float (build with -ffp-contract=off), operation by
// operation after the lines cited.  The reference computes in CV_32F with cv::SVD: results agree with it to float rounding and
// are NOT bit-identical to the CV_32F cv::SVD path.
//
// The 3 x 3 SVD A = U diag(w) V^T with full, proper U and V is jacobi_svd3 of jacobi_math.h, which says how U is completed
// for the rank-2 E21.  The signs of (u_i, v_i) are free, as in any SVD; they permute the hypotheses (H: 0 <-> 2 and 1 <-> 3
// within each group of four; F: t <-> -t, R1 <-> R2) and leave the set unchanged.
//
// The 4 x 4 null vector of Triangulate (:829-842) is jacobi_null4 of jacobi_math.h, the very routine of the triangulation of
// LocalMapping.  Every comparison of CheckRT is written as the reference writes it, so that NaN falls through the same branches.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "initializer_math.h"  // kInitH / kInitF
#include "jacobi_math.h"       // jacobi_svd3, jacobi_null4; g2o_mul3, g2o_transpose3 of g2o_math.h

namespace orbfe {

enum ReconHypStatus { kReconOk = 0, kReconNonfinite = 1 };          // ORBFE_RECON_OK / _NONFINITE
enum ReconProblemStatus { kReconProblemOk = 0, kReconDegenerate = 1 };  // ORBFE_RECON_PROBLEM_OK / _DEGENERATE
enum ReconPairFlag { kReconCounted = 1, kReconGood = 2 };           // pair_flags: the pair added 1 to nGood; vbGood

constexpr double kReconCosTh = 0.99998;   // :977, :983, :1014
constexpr double kReconSvTh = 1.00001;    // :684
constexpr int kReconSelIndex = 50;        // :1022
constexpr uint64_t kReconNoKey = ~(uint64_t)0;  // the key of a pair that takes no part in the selection

// a problem (one ReconstructH or ReconstructF) of a call.  Laid out by initializer_host.h, read by k_init_reconstruct.hip
struct ReconProblem {
  int pair0, nPairs;  // pairs [pair0, pair0 + nPairs)
  int word0;          // its ceil(nPairs / 32) inlier words
  int hyp0, nHyp;     // its hypotheses [hyp0, hyp0 + nHyp): 8 (H) or 4 (F)
  int slot0;          // its per-(hypothesis, pair) records [slot0, slot0 + nHyp * nPairs), hypothesis-major
  int kind;           // kInitH / kInitF
  float sigma;
  float K[4];         // fx fy cx cy
  double model[9];    // H21 / F21 row-major
};

ORBFE_HD inline int recon_hyps(int kind) { return kind == kInitH ? 8 : 4; }

ORBFE_HD inline double recon_det3(const double M[9]) {
  return M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
}

// Stands where the reference has cv::SVD::compute(A, w, U, Vt, FULL_UV) (:673) and cv::SVD::compute(E, w, u, vt) (:1037)
ORBFE_HD inline void recon_svd3(const double A[9], double U[9], double w[3], double V[9]) { jacobi_svd3(A, U, w, V); }

// Hypothesis `hi` of ReconstructH (:667-775): 0-3 the case d' = d2, 4-7 the case d' = -d2, in the reference's index order
// (x1 = {+,+,-,-} aux1, x3 = {+,-,+,-} aux3, stheta / sphi = {+,-,-,+} aux).  vn is never read by the reference and is not
// computed.  Returns true when `d1/d2 < 1.00001 || d2/d3 < 1.00001` (:684) holds, as written: a NaN or inf ratio is not below
// the bound.  R and t are then untouched.
ORBFE_HD inline bool recon_motion_h(const double H21[9], const float K4[4], int hi, double R[9], double t[3]) {
  const double fx = (double)K4[0], fy = (double)K4[1], cx = (double)K4[2], cy = (double)K4[3];
  const double K[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
  const double invK[9] = {1.0 / fx, 0.0, -cx / fx, 0.0, 1.0 / fy, -cy / fy, 0.0, 0.0, 1.0};  // K.inv() in closed form (:667)
  double tmp[9], A[9], U[9], V[9], Vt[9], w[3];
  g2o_mul3(invK, H21, tmp);
  g2o_mul3(tmp, K, A);  // :668
  recon_svd3(A, U, w, V);
  g2o_transpose3(V, Vt);
  const double s = recon_det3(U) * recon_det3(V);  // :677
  const double d1 = w[0], d2 = w[1], d3 = w[2];
  if (d1 / d2 < kReconSvTh || d2 / d3 < kReconSvTh) return true;  // :684
  const double aux1 = sqrt((d1 * d1 - d2 * d2) / (d1 * d1 - d3 * d3));  // :697
  const double aux3 = sqrt((d2 * d2 - d3 * d3) / (d1 * d1 - d3 * d3));  // :698
  const int i = hi & 3;
  const double e1 = (i & 2) ? -1.0 : 1.0, e3 = (i & 1) ? -1.0 : 1.0;
  const double x1 = e1 * aux1, x3 = e3 * aux3;  // :699-700
  double Rp[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, tp[3];
  if (hi < 4) {
    const double aux_stheta = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 + d3) * d2);  // :703
    const double ctheta = (d2 * d2 + d1 * d3) / ((d1 + d3) * d2);                                  // :705
    const double stheta = (e1 * e3) * aux_stheta;                                                  // :706
    Rp[0] = ctheta; Rp[2] = -stheta; Rp[6] = stheta; Rp[8] = ctheta;  // :711-714
    tp[0] = x1 * (d1 - d3); tp[1] = 0.0 * (d1 - d3); tp[2] = -x3 * (d1 - d3);  // :720-723
  } else {
    const double aux_sphi = sqrt((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)) / ((d1 - d3) * d2);  // :740
    const double cphi = (d1 * d3 - d2 * d2) / ((d1 - d3) * d2);                                  // :742
    const double sphi = (e1 * e3) * aux_sphi;                                                    // :743
    Rp[0] = cphi; Rp[2] = sphi; Rp[4] = -1.0; Rp[6] = sphi; Rp[8] = -cphi;  // :748-752
    tp[0] = x1 * (d1 + d3); tp[1] = 0.0 * (d1 + d3); tp[2] = x3 * (d1 + d3);  // :758-761
  }
  double URp[9], URpVt[9];
  g2o_mul3(U, Rp, URp);
  g2o_mul3(URp, Vt, URpVt);
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = s * URpVt[k];  // :716, :754
  const double tx = U[0] * tp[0] + U[1] * tp[1] + U[2] * tp[2];  // :725, :763
  const double ty = U[3] * tp[0] + U[4] * tp[1] + U[5] * tp[2];
  const double tz = U[6] * tp[0] + U[7] * tp[1] + U[8] * tp[2];
  const double nt = sqrt(tx * tx + ty * ty + tz * tz);
  t[0] = tx / nt; t[1] = ty / nt; t[2] = tz / nt;  // :726, :764
  return false;
}

// Hypothesis `hi` of ReconstructF (:546-566): (R1, t) (R2, t) (R1, -t) (R2, -t) of DecomposeE (:1034-1057)
ORBFE_HD inline void recon_motion_f(const double F21[9], const float K4[4], int hi, double R[9], double t[3]) {
  const double fx = (double)K4[0], fy = (double)K4[1], cx = (double)K4[2], cy = (double)K4[3];
  const double K[9] = {fx, 0.0, cx, 0.0, fy, cy, 0.0, 0.0, 1.0};
  const double Kt[9] = {fx, 0.0, 0.0, 0.0, fy, 0.0, cx, cy, 1.0};
  double tmp[9], E[9], U[9], V[9], Vt[9], w[3];
  g2o_mul3(Kt, F21, tmp);
  g2o_mul3(tmp, K, E);  // :546
  recon_svd3(E, U, w, V);
  g2o_transpose3(V, Vt);
  const double nt = sqrt(U[2] * U[2] + U[5] * U[5] + U[8] * U[8]);  // :1040-1041
  const double sg = (hi & 2) ? -1.0 : 1.0;                          // :554-555
  t[0] = sg * (U[2] / nt); t[1] = sg * (U[5] / nt); t[2] = sg * (U[8] / nt);
  // W (:1043-1046) for R1, W^T for R2
  const double m = (hi & 1) ? -1.0 : 1.0;
  const double W[9] = {0.0, -m, 0.0, m, 0.0, 0.0, 0.0, 0.0, 1.0};
  double UW[9];
  g2o_mul3(U, W, UW);
  g2o_mul3(UW, Vt, R);  // :1048, :1054
  if (recon_det3(R) < 0.0) {  // :1051-1052, :1055-1056
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = -R[k];
  }
}

// (R, t) of hypothesis hi of a problem; true: the problem is DEGENERATE (an H problem whose singular values fail :684) and
// nothing is evaluated.  R, t are zero then.
ORBFE_HD inline bool recon_motion(int kind, const double model[9], const float K4[4], int hi, double R[9], double t[3]) {
#pragma unroll
  for (int k = 0; k < 9; k++) R[k] = 0.0;
  t[0] = t[1] = t[2] = 0.0;
  if (kind == kInitH) return recon_motion_h(model, K4, hi, R, t);
  recon_motion_f(model, K4, hi, R, t);
  return false;
}

// what CheckRT sets up before its loop (:917-941)
struct ReconCam {
  double fx, fy, cx, cy;
  double R[9], t[3];
  double P2[12];  // K [R | t]
  double O2[3];   // -R^T t
  double th2;     // 4 sigma^2 (:563, :795)
};

ORBFE_HD inline void recon_camera(const float K4[4], const double R[9], const double t[3], float sigma, ReconCam* c) {
  c->fx = (double)K4[0]; c->fy = (double)K4[1]; c->cx = (double)K4[2]; c->cy = (double)K4[3];
#pragma unroll
  for (int k = 0; k < 9; k++) c->R[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; k++) c->t[k] = t[k];
#pragma unroll
  for (int j = 0; j < 3; j++) {  // :939
    c->P2[j] = c->fx * R[j] + c->cx * R[6 + j];
    c->P2[4 + j] = c->fy * R[3 + j] + c->cy * R[6 + j];
    c->P2[8 + j] = R[6 + j];
  }
  c->P2[3] = c->fx * t[0] + c->cx * t[2];
  c->P2[7] = c->fy * t[1] + c->cy * t[2];
  c->P2[11] = t[2];
#pragma unroll
  for (int j = 0; j < 3; j++) c->O2[j] = -(R[j] * t[0] + R[3 + j] * t[1] + R[6 + j] * t[2]);  // :941
  c->th2 = 4.0 * ((double)sigma * (double)sigma);
}

// One inlier pair of CheckRT (:950-1015), p = u1 v1 u2 v2.  Returns its flags (kReconCounted: the pair added 1 to nGood;
// kReconGood: vbGood); X = the triangulated point as it came out (whatever the flags), *cosParallax the cosine (0 when the
// point is not finite).
ORBFE_HD inline int recon_pair(const ReconCam& c, const float p[4], double X[3], double* cosParallax) {
  const double u1 = (double)p[0], v1 = (double)p[1], u2 = (double)p[2], v2 = (double)p[3];
  double a[16];  // :834-837 with P1 = K [I | 0]
  a[0] = -c.fx; a[1] = 0.0;   a[2] = u1 - c.cx; a[3] = 0.0;
  a[4] = 0.0;   a[5] = -c.fy; a[6] = v1 - c.cy; a[7] = 0.0;
#pragma unroll
  for (int j = 0; j < 4; j++) {
    a[8 + j] = u2 * c.P2[8 + j] - c.P2[j];
    a[12 + j] = v2 * c.P2[8 + j] - c.P2[4 + j];
  }
  double h[4];
  jacobi_null4(a, h, JacobiWaveDone());  // :840-841 (sweeps end with the wave, as in k_triangulate)
  X[0] = h[0] / h[3]; X[1] = h[1] / h[3]; X[2] = h[2] / h[3];  // :842
  *cosParallax = 0.0;
  if (!isfinite(X[0]) || !isfinite(X[1]) || !isfinite(X[2])) return 0;  // :958-962
  const double dist1 = sqrt(X[0] * X[0] + X[1] * X[1] + X[2] * X[2]);    // :965-966 (O1 = 0)
  const double n2x = X[0] - c.O2[0], n2y = X[1] - c.O2[1], n2z = X[2] - c.O2[2];  // :968
  const double dist2 = sqrt(n2x * n2x + n2y * n2y + n2z * n2z);
  const double cosP = (X[0] * n2x + X[1] * n2y + X[2] * n2z) / (dist1 * dist2);  // :972
  *cosParallax = cosP;
  if (X[2] <= 0.0 && cosP < kReconCosTh) return 0;  // :977
  const double x2 = c.R[0] * X[0] + c.R[1] * X[1] + c.R[2] * X[2] + c.t[0];  // :981
  const double y2 = c.R[3] * X[0] + c.R[4] * X[1] + c.R[5] * X[2] + c.t[1];
  const double z2 = c.R[6] * X[0] + c.R[7] * X[1] + c.R[8] * X[2] + c.t[2];
  if (z2 <= 0.0 && cosP < kReconCosTh) return 0;  // :983
  const double invZ1 = 1.0 / X[2];  // :988
  const double im1x = c.fx * X[0] * invZ1 + c.cx, im1y = c.fy * X[1] * invZ1 + c.cy;
  const double squareError1 = (im1x - u1) * (im1x - u1) + (im1y - v1) * (im1y - v1);  // :992
  if (squareError1 > c.th2) return 0;  // :995
  const double invZ2 = 1.0 / z2;  // :1000
  const double im2x = c.fx * x2 * invZ2 + c.cx, im2y = c.fy * y2 * invZ2 + c.cy;
  const double squareError2 = (im2x - u2) * (im2x - u2) + (im2y - v2) * (im2y - v2);  // :1004
  if (squareError2 > c.th2) return 0;  // :1006
  return kReconCounted | (cosP < kReconCosTh ? kReconGood : 0);  // :1010-1015
}

// an order-preserving 64-bit key of a finite double (a < b  <=>  key(a) < key(b); -0.0 before +0.0) and its inverse.  No
// finite double has the key kReconNoKey.
ORBFE_HD inline uint64_t recon_key(double c) {
  uint64_t b;
  __builtin_memcpy(&b, &c, 8);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
ORBFE_HD inline double recon_unkey(uint64_t k) {
  const uint64_t b = (k >> 63) ? (k & 0x7FFFFFFFFFFFFFFFull) : ~k;
  double c;
  __builtin_memcpy(&c, &b, 8);
  return c;
}
// the key a pair takes part in the selection with: counted and its cosine finite
ORBFE_HD inline uint64_t recon_sel_key(int flags, double cosP) {
  return ((flags & kReconCounted) && isfinite(cosP)) ? recon_key(cosP) : kReconNoKey;
}
// one step of the bisection for the key of rank `rank` (0-based, ascending): bit b of the answer, given its bits above b in
// `prefix` and count = #{keys <= prefix | (2^b - 1)}
ORBFE_HD inline uint64_t recon_bisect_probe(uint64_t prefix, int b) { return prefix | (((uint64_t)1 << b) - 1); }

// One hypothesis on the host, pair by pair as the kernel's lanes do: the kernel's arithmetic; the counts are integers and the
// selected cosine does not depend on how it is found.  pairs = the problem's [n][4], words its inlier words; x3d [n * 3],
// flags [n], keys [n] (scratch).  *degenerate as recon_motion returns it.
inline void recon_hypothesis_host(const ReconProblem& P, const float* pairs, const uint32_t* words, int hi, double R[9], double t[3],
                                  int32_t* nGood, double* cosSel, uint8_t* status, double* x3d, uint8_t* flags, uint64_t* keys,
                                  bool* degenerate, int32_t* nInliers) {
  const bool deg = recon_motion(P.kind, P.model, P.K, hi, R, t);
  ReconCam cam;
  recon_camera(P.K, R, t, P.sigma, &cam);
  int good = 0, sel = 0, inl = 0;
  for (int i = 0; i < P.nPairs; i++) {
    const bool in = ((words[i >> 5] >> (i & 31)) & 1u) != 0;
    inl += in ? 1 : 0;
    double X[3] = {0.0, 0.0, 0.0}, cosP = 0.0;
    int f = 0;
    if (in && !deg) f = recon_pair(cam, pairs + 4 * (size_t)i, X, &cosP);
    keys[i] = recon_sel_key(f, cosP);
    flags[i] = (uint8_t)f;
    x3d[3 * (size_t)i] = X[0]; x3d[3 * (size_t)i + 1] = X[1]; x3d[3 * (size_t)i + 2] = X[2];
    good += (f & kReconCounted) ? 1 : 0;
    sel += keys[i] != kReconNoKey ? 1 : 0;
  }
  double c = 0.0;
  if (sel > 0) {
    const int rank = sel - 1 < kReconSelIndex ? sel - 1 : kReconSelIndex;  // :1022
    uint64_t prefix = 0;
    for (int b = 63; b >= 0; b--) {
      const uint64_t probe = recon_bisect_probe(prefix, b);
      int cnt = 0;
      for (int i = 0; i < P.nPairs; i++) cnt += keys[i] <= probe ? 1 : 0;
      if (cnt < rank + 1) prefix |= (uint64_t)1 << b;
    }
    c = recon_unkey(prefix);
  }
  *nGood = good;
  *cosSel = c;
  *status = (uint8_t)(good != sel ? kReconNonfinite : kReconOk);
  *degenerate = deg;
  *nInliers = inl;
}

}  // namespace orbfe
