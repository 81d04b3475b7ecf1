// optsim3_math.h -- the arithmetic of Optimizer::OptimizeSim3 (src/Optimizer.cc:1116-1323), written once: k_optsim3.hip
// compiles it for the device, tests/cpp/optsim3_cpu.cpp for the host.  Plain C++ without a HIP include.  It covers the one
// graph OptimizeSim3 builds -- one free VertexSim3Expmap S12, per correspondence the two fixed points X1, X2 with an
// EdgeSim3ProjectXYZ (e12) and an EdgeInverseSim3ProjectXYZ (e21), Huber kernel, Levenberg on a dense 7 x 7 system -- from
//
// * Thirdparty/g2o/g2o/types/sim3.h (Sim3(Vector7d) :70-142, map :144-146, inverse :233-236, operator* :266-272),
// * Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h (oplusImpl :60-69, cam_map1/2 :74-88, computeError :138-145, :160-167),
// * Thirdparty/g2o/g2o/core/base_binary_edge.hpp:54-120 (constructQuadraticForm), robust_kernel_impl.cpp:78-91 (Huber; g2o_math.h),
// * Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189 and Eigen's Quaternion <-> matrix conversions.
//
// Arithmetic is binary64 on inputs widened from float (build with -ffp-contract=off).  g2o differentiates these two edges
// numerically (their linearizeOplus is commented out; base_binary_edge.hpp:131-200); here the Jacobian of the same left
// update S' = Sim3(update) * S is analytic, so results agree with g2o to the accuracy of its difference quotient and are
// NOT bit-identical to it.  Everything is written on compile-time indices, fully unrolled, so that the
// 7 x 7 system and the 36 running sums stay in registers on the device.
#pragma once
#include "g2o_math.h"

namespace orbfe {

constexpr int kOptSim3Sums = 36;  // 28 upper-triangle entries of H (row-major), 7 of b, the robust chi2
constexpr int kOptSim3MinPairs = 10;  // nCorrespondences - nBad < 10 returns 0 (src/Optimizer.cc:1293)

// g2o::Sim3's own members: r (x y z w), t, s
struct OptSim3 {
  double q[4], t[3], s;
};
struct OptSim3Cam {
  double fx, fy, cx, cy;
};
// one correspondence: X1 in camera 1, X2 in camera 2, the two observations and informations
struct OptSim3Pair {
  double X1[3], X2[3], o1[2], o2[2], w1, w2;
};
// what a pass over the pairs evaluates them at: S12, its inverse, and M = (1 / s) R^T of the e21 Jacobian
struct OptSim3Eval {
  OptSim3 S, Sinv;
  double M[9];
};

// One problem (loop candidate) of a call, as optsim3_host.h lays it out and k_optsim3.hip reads it: pairs [off, off + n)
struct OptSim3Problem {
  int32_t off, n;
  float cam1[4], cam2[4];  // fx fy cx cy
  float sim3[13];          // the incoming S12: R row-major, t, s
  float th2, delta;        // delta = sqrt(th2) as a float: const float deltaHuber (src/Optimizer.cc:1168)
  int32_t fixScale;
};
// what a problem yields besides its per-pair arrays
struct OptSim3Result {
  double sim3[8];  // qx qy qz qw tx ty tz s
  double lambda[2], chi2[2];
  int32_t nIn, nBad, rounds, pad;
  int32_t iterations[2], trials[2];
};

// the three float4 records of a pair: A = (X1, invSigma2_1), B = (X2, invSigma2_2), C = (obs1, obs2), widened
ORBFE_HD inline void optsim3_unpack(const float A[4], const float B[4], const float C[4], OptSim3Pair* p) {
  p->X1[0] = (double)A[0]; p->X1[1] = (double)A[1]; p->X1[2] = (double)A[2]; p->w1 = (double)A[3];
  p->X2[0] = (double)B[0]; p->X2[1] = (double)B[1]; p->X2[2] = (double)B[2]; p->w2 = (double)B[3];
  p->o1[0] = (double)C[0]; p->o1[1] = (double)C[1]; p->o2[0] = (double)C[2]; p->o2[1] = (double)C[3];
}

// the sim3[13] record of orbfe_sim3_ransac_multi (R row-major, t, s; floats) as the reference converts it:
// Converter::toMatrix3d / toVector3d widen, then Sim3(Matrix3d, Vector3d, double) (sim3.h:64-67; src/LoopClosing.cc:381)
ORBFE_HD inline void optsim3_from_record(const float rec[13], OptSim3* S) {
  const double R[9] = {(double)rec[0], (double)rec[1], (double)rec[2], (double)rec[3], (double)rec[4],
                       (double)rec[5], (double)rec[6], (double)rec[7], (double)rec[8]};
  g2o_quat_from_R(R, S->q);
  S->t[0] = (double)rec[9]; S->t[1] = (double)rec[10]; S->t[2] = (double)rec[11];
  S->s = (double)rec[12];
}

// Sim3(const Vector7d&) (sim3.h:70-142), branch by branch: update = (omega, upsilon, sigma).  r = Quaterniond(R) is not
// normalised afterwards
ORBFE_HD inline void optsim3_exp(const double u[7], OptSim3* out) {
  const double wx = u[0], wy = u[1], wz = u[2], sigma = u[6];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double Om[9] = {0.0, -wz, wy, wz, 0.0, -wx, -wy, wx, 0.0};
  double Om2[9], R[9];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Om2[3 * r + c] = (Om[3 * r] * Om[c] + Om[3 * r + 1] * Om[3 + c]) + Om[3 * r + 2] * Om[6 + c];
  const double s = exp(sigma);
  const double eps = 0.00001;
  double A, B, C;
  bool small;  // R = I + Omega + Omega^2
  if (fabs(sigma) < eps) {
    C = 1.0;
    if (theta < eps) {
      A = 1.0 / 2.0;
      B = 1.0 / 6.0;
      small = true;
    } else {
      const double theta2 = theta * theta;
      A = (1.0 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
      small = false;
    }
  } else {
    C = (s - 1.0) / sigma;
    if (theta < eps) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1.0) * s + 1.0) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.0) * s) / (sigma2 * sigma);
      small = true;
    } else {
      const double a = s * sin(theta);
      const double b = s * cos(theta);
      const double theta2 = theta * theta;
      const double sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
      small = false;
    }
  }
  if (small) {
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + Om[k]) + Om2[k];
  } else {
    const double ra = sin(theta) / theta, rb = (1.0 - cos(theta)) / (theta * theta);
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0 ? 1.0 : 0.0) + ra * Om[k]) + rb * Om2[k];
  }
  g2o_quat_from_R(R, out->q);
  double W[9];
#pragma unroll
  for (int k = 0; k < 9; k++) W[k] = (A * Om[k] + B * Om2[k]) + C * (k % 4 == 0 ? 1.0 : 0.0);
#pragma unroll
  for (int r = 0; r < 3; r++) out->t[r] = (W[3 * r] * u[3] + W[3 * r + 1] * u[4]) + W[3 * r + 2] * u[5];
  out->s = s;
}

// Sim3::operator* (sim3.h:266-272): r = a.r * b.r (Eigen quat_product, no normalisation); t = a.s (a.r * b.t) + a.t
ORBFE_HD inline void optsim3_mul(const OptSim3& a, const OptSim3& b, OptSim3* out) {
  double r[3];
  g2o_quat_rotate(a.q, b.t[0], b.t[1], b.t[2], r);
  g2o_quat_mul(a.q, b.q, out->q);
  out->t[0] = a.s * r[0] + a.t[0]; out->t[1] = a.s * r[1] + a.t[1]; out->t[2] = a.s * r[2] + a.t[2];
  out->s = a.s * b.s;
}

// Sim3::map (sim3.h:144-146): s (r * xyz) + t
ORBFE_HD inline void optsim3_map(const OptSim3& S, const double X[3], double P[3]) {
  double r[3];
  g2o_quat_rotate(S.q, X[0], X[1], X[2], r);
  P[0] = S.s * r[0] + S.t[0]; P[1] = S.s * r[1] + S.t[1]; P[2] = S.s * r[2] + S.t[2];
}

// Sim3::inverse (sim3.h:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
ORBFE_HD inline void optsim3_inverse(const OptSim3& S, OptSim3* out) {
  out->q[0] = -S.q[0]; out->q[1] = -S.q[1]; out->q[2] = -S.q[2]; out->q[3] = S.q[3];
  const double k = -1.0 / S.s;
  g2o_quat_rotate(out->q, k * S.t[0], k * S.t[1], k * S.t[2], out->t);
  out->s = 1.0 / S.s;
}

ORBFE_HD inline void optsim3_eval_at(const OptSim3& S, OptSim3Eval* E) {
  E->S = S;
  optsim3_inverse(S, &E->Sinv);
  double R[9];
  g2o_quat_to_R(E->Sinv.q, R);
#pragma unroll
  for (int k = 0; k < 9; k++) E->M[k] = E->Sinv.s * R[k];
}

// computeError + chi2 of e12 (types_seven_dof_expmap.h:138-145): obs1 - cam_map1(project(S12.map(X2))); chi2 = e . (w I) e
ORBFE_HD inline double optsim3_edge12(const OptSim3Eval& E, const OptSim3Cam& K1, const OptSim3Pair& p, double e[2], double P[3]) {
  optsim3_map(E.S, p.X2, P);
  e[0] = p.o1[0] - ((P[0] / P[2]) * K1.fx + K1.cx);
  e[1] = p.o1[1] - ((P[1] / P[2]) * K1.fy + K1.cy);
  return e[0] * (p.w1 * e[0]) + e[1] * (p.w1 * e[1]);
}

// computeError + chi2 of e21 (:160-167): obs2 - cam_map2(project(S12.inverse().map(X1)))
ORBFE_HD inline double optsim3_edge21(const OptSim3Eval& E, const OptSim3Cam& K2, const OptSim3Pair& p, double e[2], double P[3]) {
  optsim3_map(E.Sinv, p.X1, P);
  e[0] = p.o2[0] - ((P[0] / P[2]) * K2.fx + K2.cx);
  e[1] = p.o2[1] - ((P[1] / P[2]) * K2.fy + K2.cy);
  return e[0] * (p.w2 * e[0]) + e[1] * (p.w2 * e[1]);
}

// d e12 / d update at update = 0 of S' = Sim3(update) * S: P' = P + omega x P + upsilon + sigma P, and the projection does
// not see the scale of P: column 6 is exactly 0
ORBFE_HD inline void optsim3_jac12(const OptSim3Cam& K1, const double P[3], double J0[7], double J1[7]) {
  const double x = P[0], y = P[1];
  const double invz = 1.0 / P[2], invz_2 = invz * invz;
  J0[0] = x * y * invz_2 * K1.fx;
  J0[1] = -(1.0 + (x * x * invz_2)) * K1.fx;
  J0[2] = y * invz * K1.fx;
  J0[3] = -invz * K1.fx;
  J0[4] = 0.0;
  J0[5] = x * invz_2 * K1.fx;
  J0[6] = 0.0;
  J1[0] = (1.0 + y * y * invz_2) * K1.fy;
  J1[1] = -x * y * invz_2 * K1.fy;
  J1[2] = -x * invz * K1.fy;
  J1[3] = 0.0;
  J1[4] = -invz * K1.fy;
  J1[5] = y * invz_2 * K1.fy;
  J1[6] = 0.0;
}

// d e21 / d update: S'^-1 = S^-1 Sim3(-update), P' = S^-1.map(X1 - omega x X1 - upsilon - sigma X1), so
// dP = M [ [X1]x | -I | -X1 ] with M = (1 / s) R^T
ORBFE_HD inline void optsim3_jac21(const OptSim3Eval& E, const OptSim3Cam& K2, const double X[3], const double P[3], bool fixScale,
                                   double J0[7], double J1[7]) {
  const double x = P[0], y = P[1];
  const double invz = 1.0 / P[2], invz_2 = invz * invz;
  const double d00 = -invz * K2.fx, d02 = x * invz_2 * K2.fx;
  const double d11 = -invz * K2.fy, d12 = y * invz_2 * K2.fy;
  const double* M = E.M;
  double G[3][7];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    G[r][0] = M[3 * r + 1] * X[2] - M[3 * r + 2] * X[1];
    G[r][1] = M[3 * r + 2] * X[0] - M[3 * r] * X[2];
    G[r][2] = M[3 * r] * X[1] - M[3 * r + 1] * X[0];
    G[r][3] = -M[3 * r];
    G[r][4] = -M[3 * r + 1];
    G[r][5] = -M[3 * r + 2];
    G[r][6] = -((M[3 * r] * X[0] + M[3 * r + 1] * X[1]) + M[3 * r + 2] * X[2]);
  }
#pragma unroll
  for (int c = 0; c < 7; c++) {
    J0[c] = d00 * G[0][c] + d02 * G[2][c];
    J1[c] = d11 * G[1][c] + d12 * G[2][c];
  }
  if (fixScale) {  // VertexSim3Expmap::oplusImpl zeroes update[6] (:64-65): the error does not move along it
    J0[6] = 0.0;
    J1[6] = 0.0;
  }
}

// constructQuadraticForm (base_binary_edge.hpp:91-113) of one edge into the running sums: H += J^T (rho1 w I) J,
// b += rho1 J^T w e (negated once, after the sum), chi2 += rho0
ORBFE_HD inline void optsim3_accumulate(double (&acc)[kOptSim3Sums], const double J0[7], const double J1[7], const double e[2],
                                        double w, double rho0, double rho1) {
  const double wr = rho1 * w;
  const double we0 = wr * e[0], we1 = wr * e[1];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 7; r++)
#pragma unroll
    for (int c = r; c < 7; c++) {
      acc[k] = acc[k] + ((J0[r] * wr) * J0[c] + (J1[r] * wr) * J1[c]);
      k++;
    }
#pragma unroll
  for (int j = 0; j < 7; j++) acc[28 + j] = acc[28 + j] + (J0[j] * we0 + J1[j] * we1);
  acc[35] = acc[35] + rho0;
}

// FULL pass of one pair: both errors (chi2 out), Huber, Jacobians, e12 then e21 into the 36 sums
ORBFE_HD inline void optsim3_pair_full(const OptSim3Eval& E, const OptSim3Cam& K1, const OptSim3Cam& K2, const OptSim3Pair& p,
                                       double delta, bool fixScale, double (&acc)[kOptSim3Sums], double* chi12, double* chi21) {
  double e[2], P[3], J0[7], J1[7], rho0, rho1;
  const double c12 = optsim3_edge12(E, K1, p, e, P);
  g2o_huber(c12, delta, true, &rho0, &rho1);
  optsim3_jac12(K1, P, J0, J1);
  optsim3_accumulate(acc, J0, J1, e, p.w1, rho0, rho1);
  const double c21 = optsim3_edge21(E, K2, p, e, P);
  g2o_huber(c21, delta, true, &rho0, &rho1);
  optsim3_jac21(E, K2, p.X1, P, fixScale, J0, J1);
  optsim3_accumulate(acc, J0, J1, e, p.w2, rho0, rho1);
  *chi12 = c12;
  *chi21 = c21;
}

// TRIAL pass of one pair: both errors (chi2 out) and the robust chi2 of e12, then of e21, onto *sum
ORBFE_HD inline void optsim3_pair_trial(const OptSim3Eval& E, const OptSim3Cam& K1, const OptSim3Cam& K2, const OptSim3Pair& p,
                                        double delta, double* sum, double* chi12, double* chi21) {
  double e[2], P[3], rho0, rho1;
  const double c12 = optsim3_edge12(E, K1, p, e, P);
  g2o_huber(c12, delta, true, &rho0, &rho1);
  *sum = *sum + rho0;
  const double c21 = optsim3_edge21(E, K2, p, e, P);
  g2o_huber(c21, delta, true, &rho0, &rho1);
  *sum = *sum + rho0;
  *chi12 = c12;
  *chi21 = c21;
}

// The vertex's side of the Levenberg step (g2o_math.h: G2oLM<7>): the estimate and the trial
struct OptSim3Vertex {
  OptSim3 est, trial;
  bool fixScale;
};

// solve (H + lam I) x = b and form the trial Sim3(x) * est (VertexSim3Expmap::oplusImpl: x[6] = 0 with _fix_scale, written
// into the solver's own x, which computeScale reads afterwards)
ORBFE_HD inline void optsim3_lm_propose(G2oLM<7>* s, OptSim3Vertex* v) {
  s->ok = g2o_solve_ldlt<7>(s->S, s->lam, s->S + 28, s->x);
  if (v->fixScale) s->x[6] = 0.0;
  OptSim3 up;
  optsim3_exp(s->x, &up);
  optsim3_mul(up, v->est, &v->trial);
}

// a pair is erased when e12->chi2() > th2 || e21->chi2() > th2 (src/Optimizer.cc:1274, :1309): double against the float
// th2 widened (a NaN chi2 is kept)
ORBFE_HD inline bool optsim3_is_bad(double chi12, double chi21, float th2) { return chi12 > (double)th2 || chi21 > (double)th2; }

}  // namespace orbfe
