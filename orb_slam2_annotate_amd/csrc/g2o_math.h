// g2o_math.h -- the g2o / Eigen arithmetic the four optimisers of src/Optimizer.cc share, written once: the quaternion <->
// matrix conversions, SE3Quat's normalisation and exp(x) * est, the Huber kernel, the unpivoted LDL^T of a dense N x N
// system, the projection error of an SE3 edge and OptimizationAlgorithmLevenberg::solve for a problem of one vertex.
// poseopt_math.h, optsim3_math.h, lba_math.h and essgraph_math.h build on it; the kernels compile it for the device, the
// programs under tests/cpp for the host.  Plain C++ without a HIP include, and the one definition of ORBFE_HD.
//
// Arithmetic is binary64 (build with -ffp-contract=off): every product and sum rounds where it is written, and every
// parenthesis below is the order the results are pinned to.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#ifndef ORBFE_HD
#if defined(__HIPCC__)
#define ORBFE_HD __host__ __device__
#else
#define ORBFE_HD
#endif
#endif

namespace orbfe {

// 3 x 3, row-major.  C = A B with every entry summed left to right, as Eigen's product and cv's gemm do; T = M^T
ORBFE_HD inline void g2o_mul3(const double A[9], const double B[9], double C[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) C[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
}
ORBFE_HD inline void g2o_transpose3(const double M[9], double T[9]) {
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) T[3 * i + j] = M[3 * j + i];
}

// Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h: quaternionbase_assign_impl<Other, 3, 3>); m row-major
ORBFE_HD inline void g2o_quat_from_R(const double m[9], double q[4]) {
  double t = m[0] + m[4] + m[8];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[7] - m[5]) * t;
    q[1] = (m[2] - m[6]) * t;
    q[2] = (m[3] - m[1]) * t;
  } else {
    int i = 0;
    if (m[4] > m[0]) i = 1;
    if (m[8] > (i == 0 ? m[0] : m[4])) i = 2;
    // j = (i + 1) % 3, k = (j + 1) % 3, written out so that every index is a constant
    if (i == 0) {
      t = sqrt(m[0] - m[4] - m[8] + 1.0);
      q[0] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[7] - m[5]) * t;
      q[1] = (m[3] + m[1]) * t;
      q[2] = (m[6] + m[2]) * t;
    } else if (i == 1) {
      t = sqrt(m[4] - m[8] - m[0] + 1.0);
      q[1] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[2] - m[6]) * t;
      q[2] = (m[7] + m[5]) * t;
      q[0] = (m[1] + m[3]) * t;
    } else {
      t = sqrt(m[8] - m[0] - m[4] + 1.0);
      q[2] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[3] - m[1]) * t;
      q[0] = (m[2] + m[6]) * t;
      q[1] = (m[5] + m[7]) * t;
    }
  }
}

// SE3Quat::normalizeRotation (Thirdparty/g2o/g2o/types/se3quat.h:280-285)
ORBFE_HD inline void g2o_normalize_rotation(double q[4]) {
  if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] = q[0] / n; q[1] = q[1] / n; q[2] = q[2] / n; q[3] = q[3] / n;
}

// Eigen QuaternionBase::_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv
ORBFE_HD inline void g2o_quat_rotate(const double q[4], double X, double Y, double Z, double r[3]) {
  double uvx = q[1] * Z - q[2] * Y;
  double uvy = q[2] * X - q[0] * Z;
  double uvz = q[0] * Y - q[1] * X;
  uvx = uvx + uvx;
  uvy = uvy + uvy;
  uvz = uvz + uvz;
  r[0] = (X + q[3] * uvx) + (q[1] * uvz - q[2] * uvy);
  r[1] = (Y + q[3] * uvy) + (q[2] * uvx - q[0] * uvz);
  r[2] = (Z + q[3] * uvz) + (q[0] * uvy - q[1] * uvx);
}

// Eigen QuaternionBase::toRotationMatrix, row-major
ORBFE_HD inline void g2o_quat_to_R(const double q[4], double R[9]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1.0 - (txx + tyy);
}

// Eigen quat_product: a * b, not normalised
ORBFE_HD inline void g2o_quat_mul(const double a[4], const double b[4], double q[4]) {
  const double ax = a[0], ay = a[1], az = a[2], aw = a[3];
  const double bx = b[0], by = b[1], bz = b[2], bw = b[3];
  q[0] = aw * bx + ax * bw + ay * bz - az * by;
  q[1] = aw * by + ay * bw + az * bx - ax * bz;
  q[2] = aw * bz + az * bw + ax * by - ay * bx;
  q[3] = aw * bw - ax * bx - ay * by - az * bz;
}

// VertexSE3Expmap::oplusImpl: out = SE3Quat::exp(x) * est (se3quat.h:223-257 with its theta < 1e-5 branch, operator*
// :104-110); x = (omega, upsilon), pow(theta, 3) is taken as theta * theta * theta.  est, out: q (x y z w), then t -- the
// first 7 doubles of a record of LbaArgs::pose
ORBFE_HD inline void g2o_se3_oplus(const double x[6], const double* est, double* out) {
  const double wx = x[0], wy = x[1], wz = x[2];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double Om[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double Om2[9], R[9], V[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Om2[3 * r + c] = (Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c]) + Om[3 * r + 2] * Om[6 + c];
  if (theta < 0.00001) {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k];
      V[k] = R[k];
    }
  } else {
    const double a = sin(theta) / theta;
    const double b = (1.0 - cos(theta)) / (theta * theta);
    const double c3 = (theta - sin(theta)) / (theta * theta * theta);
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const double I = k % 4 == 0 ? 1.0 : 0.0;
      R[k] = (I + a * Om[k]) + b * Om2[k];
      V[k] = (I + b * Om[k]) + c3 * Om2[k];
    }
  }
  double qe[4], te[3], rt[3], q[4];
#pragma unroll
  for (int r = 0; r < 3; r++) te[r] = (V[3 * r] * x[3] + V[3 * r + 1] * x[4]) + V[3 * r + 2] * x[5];
  g2o_quat_from_R(R, qe);
  g2o_normalize_rotation(qe);  // SE3Quat(Quaterniond, Vector3d)
  // SE3Quat::operator*: t = a.t + a.r * b.t; r = a.r * b.r; normalizeRotation
  g2o_quat_rotate(qe, est[4], est[5], est[6], rt);
  g2o_quat_mul(qe, est, q);
  g2o_normalize_rotation(q);
  out[0] = q[0]; out[1] = q[1]; out[2] = q[2]; out[3] = q[3];
  out[4] = te[0] + rt[0]; out[5] = te[1] + rt[1]; out[6] = te[2] + rt[2];
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91): rho and its first derivative; with robust off the identity.
// (A NaN chi2 takes the identity, as in tests/pose_opt_ref.py and tests/optimize_sim3_ref.py.)
ORBFE_HD inline void g2o_huber(double chi2, double delta, bool robust, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  *rho0 = chi2;
  *rho1 = 1.0;
  if (robust && chi2 > dsqr) {
    const double sq = sqrt(chi2);
    *rho0 = 2 * sq * delta - dsqr;
    *rho1 = delta / sq;
  }
}

// (H + lam I) x = b by unpivoted LDL^T; Hs: the N (N + 1) / 2 upper-triangle entries, row-major.  false on a pivot that is
// not positive: the update is zero and the trial counts as DBL_MAX (optimization_algorithm_levenberg.cpp:126-127).  No early
// return, so that the fully unrolled elimination stays one straight line
template <int N>
ORBFE_HD inline bool g2o_solve_ldlt(const double* Hs, double lam, const double* b, double x[N]) {
  double A[N][N], L[N][N], D[N], y[N];
  int k = 0;
#pragma unroll
  for (int r = 0; r < N; r++)
#pragma unroll
    for (int c = r; c < N; c++) { A[r][c] = Hs[k]; A[c][r] = Hs[k]; k++; }
#pragma unroll
  for (int j = 0; j < N; j++) A[j][j] = A[j][j] + lam;
  bool ok = true;
#pragma unroll
  for (int j = 0; j < N; j++) {
    double d = A[j][j];
#pragma unroll
    for (int m = 0; m < j; m++) d = d - (L[j][m] * L[j][m]) * D[m];
    if (!(d > 0.0)) ok = false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < N; i++) {
      double s = A[j][i];
#pragma unroll
      for (int m = 0; m < j; m++) s = s - (L[i][m] * L[j][m]) * D[m];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < N; i++) {
    double s = b[i];
#pragma unroll
    for (int m = 0; m < i; m++) s = s - L[i][m] * y[m];
    y[i] = s;
  }
#pragma unroll
  for (int i = N - 1; i >= 0; i--) {
    double s = y[i] / D[i];
#pragma unroll
    for (int m = i + 1; m < N; m++) s = s - L[m][i] * x[m];
    x[i] = s;
  }
  if (!ok) {
#pragma unroll
    for (int i = 0; i < N; i++) x[i] = 0.0;
  }
  return ok;
}

// computeError + chi2 of an SE3 projection edge at pose P (q, then t) for the point X: SE3Quat::map (se3quat.h:217-220),
// then mono obs - (x / z * fx + cx, y / z * fy + cy), or stereo -- !(ur < 0) -- cam_project with its FLOAT invz = 1.0f / z
// (types_six_dof_expmap.cpp:141-157, :290-306).  A monocular edge is carried with a third row of zeros: adding +0.0 changes
// no sum.  K: fx fy cx cy bf.  chi2 = e . (w I) e; xyz: the point in the camera
ORBFE_HD inline double g2o_se3_project_error(const double* P, const double K[5], const double X[3], double u, double v, double ur,
                                             double w, double e[3], double xyz[3]) {
  double c[3];
  g2o_quat_rotate(P, X[0], X[1], X[2], c);
  const double x = c[0] + P[4], y = c[1] + P[5], z = c[2] + P[6];
  xyz[0] = x; xyz[1] = y; xyz[2] = z;
  if (!(ur < 0)) {
    const double invz = (double)(float)(1.0 / z);  // const float invz = 1.0f / trans_xyz[2]
    const double p0 = (x * invz) * K[0] + K[2];
    const double p1 = (y * invz) * K[1] + K[3];
    const double p2 = p0 - K[4] * invz;
    e[0] = u - p0;
    e[1] = v - p1;
    e[2] = ur - p2;
  } else {
    e[0] = u - ((x / z) * K[0] + K[2]);
    e[1] = v - ((y / z) * K[1] + K[3]);
    e[2] = 0.0;
  }
  return (e[0] * (w * e[0]) + e[1] * (w * e[1])) + e[2] * (w * e[2]);
}

// OptimizationAlgorithmLevenberg::solve (optimization_algorithm_levenberg.cpp:61-189) for a problem of ONE vertex with N
// unknowns, as two steps around the passes over the edges: g2o_lm_after_full() consumes the sums of a FULL pass at the
// estimate, g2o_lm_after_trial() the robust chi2 of a TRIAL pass at `trial`, which it copies to *est when the step is
// accepted.  Both return what runs next.  The proposal -- the solve and the vertex's oplus -- is the caller's: it follows
// after_full directly, and after_trial calls `propose` where Levenberg's loop tries the next lambda.  (Called there and not
// after the return: k_optimize_sim3 sits on the register limit, and with the proposal behind the return it came out 6 % slower.)
// (LbaLM and ess_lm_after_linearise are not copies of this: host-driven rules of multi-vertex problems on an LbaRecord.)
enum G2oLMCmd { kG2oLMDone = 0, kG2oLMFull = 1, kG2oLMTrial = 2 };

template <int N>
struct G2oLM {
  static constexpr int kH = N * (N + 1) / 2, kSums = kH + N + 1;
  double S[kSums];  // H (upper triangle, row-major), b (negated), robust chi2 of the last FULL pass
  double x[N];
  double lam, ni, cur, ini;
  int nBadLM, q, it, trials, maxIt;
  bool ok;  // of the last solve
};

// optimize(maxIt) starts: iteration 0 re-initialises lambda (:77-81)
template <int N>
ORBFE_HD inline void g2o_lm_begin(G2oLM<N>* s, int maxIt) {
  s->lam = 0.0; s->ni = 2.0; s->cur = 0.0; s->ini = 0.0;
  s->nBadLM = 0; s->q = 0; s->it = 0; s->trials = 0; s->maxIt = maxIt;
  s->ok = true;
}

template <int N>
ORBFE_HD inline int g2o_lm_after_full(G2oLM<N>* s) {
  constexpr int kH = G2oLM<N>::kH;
#pragma unroll
  for (int j = 0; j < N; j++) s->S[kH + j] = -s->S[kH + j];
  s->cur = s->ini = s->S[kH + N];
  if (s->it == 0) {  // computeLambdaInit: tau * max |H_jj| (:166-180)
    double mx = 0.0;
#pragma unroll
    for (int j = 0; j < N; j++) mx = fmax(fabs(s->S[j * N - j * (j - 1) / 2]), mx);
    s->lam = 1e-5 * mx;
    s->ni = 2.0;
    s->nBadLM = 0;
  }
  s->q = 0;
  return kG2oLMTrial;
}

// temp: the robust chi2 at the trial; V: the caller's vertex estimate
template <int N, class V, class Propose>
ORBFE_HD inline int g2o_lm_after_trial(G2oLM<N>* s, double temp, V* est, const V& trial, Propose propose) {
  if (!s->ok) temp = DBL_MAX;  // (:126-127)
  const double* b = s->S + G2oLM<N>::kH;
  double scale = 0.0;  // computeScale (:182-189)
#pragma unroll
  for (int j = 0; j < N; j++) scale = scale + s->x[j] * (s->lam * s->x[j] + b[j]);
  scale = scale + 1e-3;
  const double rho = (s->cur - temp) / scale;
  s->trials++;
  if (rho > 0 && isfinite(temp)) {  // (:134-147)
    const double tt = 2 * rho - 1;
    const double alpha = fmin(1.0 - tt * tt * tt, 2.0 / 3.0);
    s->lam = s->lam * fmax(1.0 / 3.0, alpha);
    s->ni = 2.0;
    s->cur = temp;
    *est = trial;
  } else {
    s->lam = s->lam * s->ni;
    s->ni = s->ni * 2;
  }
  s->q++;
  if (rho < 0 && s->q < 10) {  // (:149)
    propose();
    return kG2oLMTrial;
  }
  s->it++;
  bool stop = (s->q == 10 || rho == 0);  // (:151-152)
  if (!stop) {
    if ((s->ini - s->cur) * 1e3 < s->ini) s->nBadLM++;  // Stop criterium (Raul) (:154-161)
    else s->nBadLM = 0;
    stop = s->nBadLM >= 3;
  }
  return (stop || s->it == s->maxIt) ? kG2oLMDone : kG2oLMFull;
}

}  // namespace orbfe
