// sim3_math.h -- one RANSAC hypothesis of Sim3Solver: Sim3Solver::ComputeSim3 (src/Sim3Solver.cc:254-370, Horn's closed form
// on three pairs) and the per-pair test of CheckInliers / Project (:374-442), written once: k_sim3.hip compiles it for the
// device, tests/cpp/sim3_cpu.cpp and tests/cpp/sim3_host_san.cpp for the host.  Plain C++ without a HIP include.  Arithmetic
// is binary64 on inputs widened from float (build with -ffp-contract=off).  The reference computes in CV_32F with cv::eigen
// and cv::Rodrigues, so results agree with it to float rounding and are NOT bit-identical to it; a pair within float rounding
// of its maxErr may fall on the other side.  Every index is a compile-time constant (after unrolling, in jacobi_math.h's
// iteration) so that the 4 x 4 matrices stay in registers on the device.
//
// IEEE semantics the reference relies on are kept: two identical point sets make row 0 of N (0 off the diagonal), the
// eigenvector is (+-1, 0, 0, 0), |vec| = 0, the reference divides by it (:310) and everything downstream is NaN, so that
// every comparison of CheckInliers is false: 0 inliers.  Here the same division happens; sim3_nonfinite() then names the case.
// cv::Rodrigues' small-angle branch (theta < DBL_EPSILON gives the identity) is not written: theta = 2 atan2(|vec|, q0)
// is 0 only with |vec| = 0, which is that NaN (NaN < DBL_EPSILON is false, so cv::Rodrigues takes its general branch too),
// and for a |vec| so small that 0 < theta < DBL_EPSILON the general formula gives I + theta [r]x, the identity in float.
#pragma once
#include <float.h>
#include <math.h>

#include "jacobi_math.h"  // jacobi_sym_pair; ORBFE_HD

namespace orbfe {

enum Sim3Status { kSim3Ok = 0, kSim3Nonfinite = 1 };  // ORBFE_SIM3_* of include/orbfe.h

// what one hypothesis yields: R12 row-major, t12, s12 and the two transforms the inlier test reads
struct Sim3Transform {
  double R[9], t[3], s;
  double T12[12];  // [sR | t], row-major 3 x 4
  double T21[12];  // [(1/s) R^T | -(1/s) R^T t]
};
// fx fy cx cy
struct Sim3Camera {
  float fx, fy, cx, cy;
};

// a candidate (one Sim3Solver) of a call: where its pairs, hypotheses and mask words begin.  Laid out by sim3_host.h, read by
// k_sim3.hip
struct Sim3Candidate {
  int pair0, nPairs;   // pairs [pair0, pair0 + nPairs) of x3dc1 / x3dc2 / maxErr1 / maxErr2
  int hyp0;            // its first hypothesis
  int word0, words;    // mask words of its first hypothesis; words per hypothesis = ceil(nPairs / 32)
  Sim3Camera K1, K2;
};

// The eigenvector of the largest eigenvalue of the symmetric 4 x 4 `a` (row-major; destroyed): the column of V under the
// largest diagonal entry (the first of equal ones) after jacobi_math.h's two-sided iteration.  Stands where the reference has
// evec.row(0) of cv::eigen (:300); the sign is free and cancels in sim3_rotation.
ORBFE_HD inline void sim3_top_eigenvector(double a[16], double q[4]) {
  double v[16];
  jacobi_identity(v, 4);
  jacobi_sweeps_unrolled<4>([&](int p, int k) { return jacobi_sym_pair(a, v, 4, p, k); }, JacobiOwnDone());
  double best = a[0];
  q[0] = v[0]; q[1] = v[4]; q[2] = v[8]; q[3] = v[12];
  if (a[5] > best) { best = a[5]; q[0] = v[1]; q[1] = v[5]; q[2] = v[9]; q[3] = v[13]; }
  if (a[10] > best) { best = a[10]; q[0] = v[2]; q[1] = v[6]; q[2] = v[10]; q[3] = v[14]; }
  if (a[15] > best) { best = a[15]; q[0] = v[3]; q[1] = v[7]; q[2] = v[11]; q[3] = v[15]; }
}

// :302-314: the rotation from the quaternion the reference's way -- angle-axis, then cv::Rodrigues' formula
// R = cos(theta) I + (1 - cos(theta)) r r^T + sin(theta) [r]x -- so that q and -q give the same R (atan2 sees the sign of
// q0, the axis flips with it: theta' = 2 pi - theta about -r) and |vec| = 0 gives NaN
ORBFE_HD inline void sim3_rotation(const double q[4], double R[9]) {
  const double nv = sqrt(q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);  // norm(vec)
  const double ang = atan2(nv, q[0]);                               // :308
  const double k = 2.0 * ang / nv;                                  // :310 (MatExpr: vec scaled once by 2 ang / norm)
  const double rx = k * q[1], ry = k * q[2], rz = k * q[3];
  const double theta = sqrt(rx * rx + ry * ry + rz * rz);
  const double c = cos(theta), s = sin(theta), c1 = 1.0 - c, it = 1.0 / theta;
  const double x = rx * it, y = ry * it, z = rz * it;
  R[0] = c + c1 * x * x;     R[1] = c1 * x * y - s * z; R[2] = c1 * x * z + s * y;
  R[3] = c1 * x * y + s * z; R[4] = c + c1 * y * y;     R[5] = c1 * y * z - s * x;
  R[6] = c1 * x * z - s * y; R[7] = c1 * y * z + s * x; R[8] = c + c1 * z * z;
}

// Sim3Solver::ComputeSim3 (:254-370) on the three pairs P1[j] <-> P2[j] (camera coordinates of key frames 1 and 2)
ORBFE_HD inline void sim3_compute(const float P1[3][3], const float P2[3][3], bool fixScale, Sim3Transform* o) {
  // Step 1 (:259-267): centroids, relative coordinates; a[i][j] = coordinate i of pair j, as the reference's columns
  double O1[3], O2[3], a1[3][3], a2[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++) {
    O1[i] = ((double)P1[0][i] + (double)P1[1][i] + (double)P1[2][i]) / 3.0;
    O2[i] = ((double)P2[0][i] + (double)P2[1][i] + (double)P2[2][i]) / 3.0;
#pragma unroll
    for (int j = 0; j < 3; j++) { a1[i][j] = (double)P1[j][i] - O1[i]; a2[i][j] = (double)P2[j][i] - O2[i]; }
  }
  // Step 2 (:271): M = Pr2 Pr1^T
  double M[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[i][j] = a2[i][0] * a1[j][0] + a2[i][1] * a1[j][1] + a2[i][2] * a1[j][2];
  // Step 3 (:279-293)
  const double N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const double N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const double N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  double N[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
  // Step 4 (:296-314)
  double q[4];
  sim3_top_eigenvector(N, q);
  sim3_rotation(q, o->R);
  const double* R = o->R;
  // Steps 5, 6 (:319-343): P3 = R Pr2, s = Pr1 . P3 / sum P3^2, summed row by row as cv's dot and the loop of :332 do
  double s = 1.0;
  if (!fixScale) {
    double nom = 0.0, den = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        const double p3 = R[3 * i] * a2[0][j] + R[3 * i + 1] * a2[1][j] + R[3 * i + 2] * a2[2][j];
        nom += a1[i][j] * p3;
        den += p3 * p3;
      }
    s = nom / den;
  }
  o->s = s;
  // Steps 7, 8 (:347-369)
  const double is = 1.0 / s;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double r0 = s * R[3 * i], r1 = s * R[3 * i + 1], r2 = s * R[3 * i + 2];
    o->t[i] = O1[i] - (r0 * O2[0] + r1 * O2[1] + r2 * O2[2]);  // :348
    o->T12[4 * i] = r0; o->T12[4 * i + 1] = r1; o->T12[4 * i + 2] = r2; o->T12[4 * i + 3] = o->t[i];
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double r0 = is * R[i], r1 = is * R[3 + i], r2 = is * R[6 + i];  // (1/s) R^T (:365)
    o->T21[4 * i] = r0; o->T21[4 * i + 1] = r1; o->T21[4 * i + 2] = r2;
    o->T21[4 * i + 3] = -(r0 * o->t[0] + r1 * o->t[1] + r2 * o->t[2]);   // :368
  }
}

// any of R, t, s not finite: the hypothesis is ORBFE_SIM3_NONFINITE, has 0 inliers and an all-zero mask
ORBFE_HD inline bool sim3_nonfinite(const Sim3Transform& o) {
  bool ok = isfinite(o.s);
#pragma unroll
  for (int i = 0; i < 9; i++) ok = ok && isfinite(o.R[i]);
#pragma unroll
  for (int i = 0; i < 3; i++) ok = ok && isfinite(o.t[i]);
  return !ok;
}

// Sim3Solver::Project (:421-442) for one point, FromCameraToImage (:445-463) when T is NULL: no depth test, as the reference
ORBFE_HD inline void sim3_project(const double* T, const Sim3Camera& K, const float X[3], double* u, double* v) {
  double x = (double)X[0], y = (double)X[1], z = (double)X[2];
  if (T) {
    const double px = T[0] * x + T[1] * y + T[2] * z + T[3], py = T[4] * x + T[5] * y + T[6] * z + T[7];
    const double pz = T[8] * x + T[9] * y + T[10] * z + T[11];  // :435
    x = px; y = py; z = pz;
  }
  const double invz = 1.0 / z;  // :436
  *u = (double)K.fx * (x * invz) + (double)K.cx;  // :437-440
  *v = (double)K.fy * (y * invz) + (double)K.cy;
}

// CheckInliers (:382-397) for one pair: X1 / X2 = the pair in the cameras of key frames 1 / 2
ORBFE_HD inline bool sim3_is_inlier(const Sim3Transform& o, const Sim3Camera& K1, const Sim3Camera& K2, const float X1[3],
                                    const float X2[3], float maxErr1, float maxErr2) {
  double u11, v11, u22, v22, u21, v21, u12, v12;
  sim3_project(nullptr, K1, X1, &u11, &v11);  // mvP1im1 (:108)
  sim3_project(nullptr, K2, X2, &u22, &v22);  // mvP2im2 (:109)
  sim3_project(o.T12, K1, X2, &u21, &v21);    // vP2im1 (:377)
  sim3_project(o.T21, K2, X1, &u12, &v12);    // vP1im2 (:378)
  const double e1 = (u11 - u21) * (u11 - u21) + (v11 - v21) * (v11 - v21);  // :384, :387
  const double e2 = (u12 - u22) * (u12 - u22) + (v12 - v22) * (v12 - v22);  // :385, :388
  return e1 < (double)maxErr1 && e2 < (double)maxErr2;                      // :390
}

}  // namespace orbfe
