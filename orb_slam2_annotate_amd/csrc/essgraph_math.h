// essgraph_math.h -- the arithmetic of Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:833-1104), written once:
// k_essgraph.hip compiles it for the device, tests/cpp/essgraph_cpu.cpp for the host.  Plain C++ without a HIP include.  It
// covers the one graph OptimizeEssentialGraph builds -- a VertexSim3Expmap per key frame (free, or fixed for the loop key
// frame), an EdgeSim3 with identity information and no robust kernel per spanning-tree / loop / covisibility link,
// Levenberg with lambda_init = 1e-16 on the full 7 n x 7 n system, nothing marginalised -- from
//
// * Thirdparty/g2o/g2o/types/sim3.h (log :148-230, and through optsim3_math.h: Sim3(Vector7d), map, inverse, operator*),
// * Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h (oplusImpl :60-69, EdgeSim3::computeError :106-114),
// * Thirdparty/g2o/g2o/types/se3_ops.hpp (deltaR, skew), Eigen's PartialPivLU for the 3 x 3 solve of log,
// * Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189 (through lba_math.h: LbaLM).
//
// Arithmetic is binary64 (build with -ffp-contract=off).  g2o differentiates EdgeSim3 numerically with delta 1e-9; here the
// Jacobians of the same left update S' = Sim3(update) * S are analytic: with E = C S_i S_j^-1 and
// e = log E,  J_j = -G,  J_i = G Ad(S_j S_i^-1),  G = d log(E Sim3(xi)) / d xi of Sim3::log AS IT IS COMPUTED, branch by branch
// (ess_log_jacobian).  Where the branches of log are exact G is Jr^-1(e); where they freeze a coefficient or, as sim3.h:199,
// depart from the closed form, G follows what is computed, because that is what g2o's difference quotient differentiates.
//
// Three layers: the Sim3 arithmetic, the WORK ITEMS of the kernels (ess_*: what one lane does on the arrays of EssArgs) and
// the element operations of the block-sparse Cholesky (7 x 7 blocks, block-CSC lower triangle).  Every element of the factor
// has one owner per step and takes its updates in ascending column order, so the device and the CPU program give the same
// factor bit for bit (only + - x / sqrt are used there).
#pragma once
#include <float.h>
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "lba_math.h"      // LbaRecord, LbaLM and the Levenberg rules, unmodified
#include "optsim3_math.h"  // OptSim3, optsim3_exp / _mul / _inverse / _map, unmodified; g2o_quat_to_R through it

namespace orbfe {

constexpr int kEssLanes = 64;
constexpr int kEssLin = 105;  // doubles per edge of EssArgs::lin: e 7 | J_i 49 | J_j 49 (row-major 7 x 7)
constexpr double kEssLambdaInit = 1e-16;  // setUserLambdaInit(1e-16) (src/Optimizer.cc:847)

// The arrays of a call.  Vertices keep the caller's order; the free ones have an index f in [0, nFree) in that order, which
// is the order of the block columns.  Estimates are kept twice, [0] and [1]: the estimate and the trial of the current step.
struct EssArgs {
  int32_t nVertices, nFree, nEdges, nActive, blocksA, blocksL, fixScale, pad;
  const double* sim3;         // [nVertices][8]: qx qy qz qw tx ty tz s (vScw)
  const double* sim3Meas;     // [nVertices][8]: Snc
  const int32_t* freeOf;      // [nVertices]: f or -1
  const int32_t* freeVertex;  // [nFree]
  const int32_t* edgeI;       // [nEdges]: vertex 0 of the edge
  const int32_t* edgeJ;       // [nEdges]: vertex 1
  const uint8_t* edgeKind;    // [nEdges]: 0 measurement from sim3Meas, 1 from sim3
  const int32_t* activeEdge;  // [nActive]: the edges with a free vertex, ascending
  const int32_t* colptr;      // [nFree + 1]: block columns of the factor's pattern; the first block of a column is its diagonal
  const int32_t* rowidx;      // [blocksL]: block rows, ascending within a column
  const int32_t* blockCol;    // [blocksL]
  const int32_t* itemBlock;   // [blocksA]: the blocks of H that have edges (the others are fill)
  const int32_t* itemOff;     // [blocksA + 1]: CSR over itemEdge
  const int32_t* itemEdge;    // diagonal block: the active edges of the vertex; off-diagonal: the edges of the pair; ascending
  const int32_t* updOff;      // [blocksL + 1]: CSR over updSrc
  const int32_t* updSrc;      // [.][2]: blocks (i, k) and (j, k) that update block (i, j), k ascending
  double* est;                // [2][nVertices][8]
  double* meas;               // [nEdges][8]: Sji
  double* lin;                // [nEdges][kEssLin]
  double* chi2;               // [nEdges]: of the last evaluation
  double* H;                  // [blocksL][49] row-major blocks; fill blocks stay 0
  double* b;                  // [nFree][7]
  double* L;                  // [blocksL][49]: H + lambda I, then its Cholesky factor
  double* x;                  // [nFree][7]: b, then the step
  LbaRecord* rec;
};

ORBFE_HD inline void ess_load(const double* rec8, OptSim3* S) {
  S->q[0] = rec8[0]; S->q[1] = rec8[1]; S->q[2] = rec8[2]; S->q[3] = rec8[3];
  S->t[0] = rec8[4]; S->t[1] = rec8[5]; S->t[2] = rec8[6];
  S->s = rec8[7];
}
ORBFE_HD inline void ess_store(const OptSim3& S, double* rec8) {
  rec8[0] = S.q[0]; rec8[1] = S.q[1]; rec8[2] = S.q[2]; rec8[3] = S.q[3];
  rec8[4] = S.t[0]; rec8[5] = S.t[1]; rec8[6] = S.t[2];
  rec8[7] = S.s;
}

// ---------------------------------------------------------------------------------------------------------------------
// 3 x 3 helpers, row-major, every sum in index order
ORBFE_HD inline void ess_mulv3(const double A[9], const double v[3], double o[3]) {
#pragma unroll
  for (int r = 0; r < 3; r++) o[r] = (A[3 * r] * v[0] + A[3 * r + 1] * v[1]) + A[3 * r + 2] * v[2];
}
ORBFE_HD inline void ess_skew(const double v[3], double M[9]) {
  M[0] = 0.0; M[1] = -v[2]; M[2] = v[1];
  M[3] = v[2]; M[4] = 0.0; M[5] = -v[0];
  M[6] = -v[1]; M[7] = v[0]; M[8] = 0.0;
}
template <int N>
ORBFE_HD inline void ess_swap_rows(double* a, double* b) {
#pragma unroll
  for (int k = 0; k < N; k++) { const double t = a[k]; a[k] = b[k]; b[k] = t; }
}
// M X = B by elimination with partial pivoting (the first largest |entry| of the column, as Eigen's PartialPivLU picks it);
// B is 3 x N row-major and is overwritten by X
template <int N>
ORBFE_HD inline void ess_solve3(const double M[9], double* B) {
  double a[9];
#pragma unroll
  for (int k = 0; k < 9; k++) a[k] = M[k];
  {
    int p = 0;
    if (fabs(a[3]) > fabs(a[0])) p = 1;
    if (fabs(a[6]) > fabs(p == 0 ? a[0] : a[3])) p = 2;
    if (p == 1) { ess_swap_rows<3>(a, a + 3); ess_swap_rows<N>(B, B + N); }
    else if (p == 2) { ess_swap_rows<3>(a, a + 6); ess_swap_rows<N>(B, B + 2 * N); }
  }
  const double l1 = a[3] / a[0], l2 = a[6] / a[0];
  a[4] = a[4] - l1 * a[1]; a[5] = a[5] - l1 * a[2];
  a[7] = a[7] - l2 * a[1]; a[8] = a[8] - l2 * a[2];
#pragma unroll
  for (int k = 0; k < N; k++) { B[N + k] = B[N + k] - l1 * B[k]; B[2 * N + k] = B[2 * N + k] - l2 * B[k]; }
  if (fabs(a[7]) > fabs(a[4])) {
    { double t = a[4]; a[4] = a[7]; a[7] = t; t = a[5]; a[5] = a[8]; a[8] = t; }
    ess_swap_rows<N>(B + N, B + 2 * N);
  }
  const double l3 = a[7] / a[4];
  a[8] = a[8] - l3 * a[5];
#pragma unroll
  for (int k = 0; k < N; k++) {
    B[2 * N + k] = B[2 * N + k] - l3 * B[N + k];
    const double x2 = B[2 * N + k] / a[8];
    const double x1 = (B[N + k] - a[5] * x2) / a[4];
    const double x0 = ((B[k] - a[1] * x1) - a[2] * x2) / a[0];
    B[k] = x0; B[N + k] = x1; B[2 * N + k] = x2;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// which branch Sim3::log took and what the Jacobian needs of it: theta, the coefficients, W (upsilon = W^-1 t) and R
struct EssLogBranch {
  bool smallSigma, smallTheta;
  double theta, A, B, C, W[9], R[9];
};

// Sim3::log (sim3.h:148-230), branch by branch: (omega, upsilon, sigma).  R = r.toRotationMatrix() of the quaternion as it is
ORBFE_HD inline void essgraph_log_ex(const OptSim3& S, double out[7], EssLogBranch& br) {
  const double sigma = log(S.s);
  double R[9];
  g2o_quat_to_R(S.q, R);
  const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
  const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};  // deltaR (se3_ops.hpp)
  const double eps = 0.00001;
  double w[3], A, B, C, theta = 0.0;
  if (fabs(sigma) < eps) {
    C = 1.0;
    if (d > 1.0 - eps) {
      w[0] = 0.5 * dR[0]; w[1] = 0.5 * dR[1]; w[2] = 0.5 * dR[2];
      A = 1.0 / 2.0;
      B = 1.0 / 6.0;
    } else {
      theta = acos(d);
      const double theta2 = theta * theta;
      const double k = theta / (2.0 * sqrt(1.0 - d * d));
      w[0] = k * dR[0]; w[1] = k * dR[1]; w[2] = k * dR[2];
      A = (1.0 - cos(theta)) / theta2;
      B = (theta - sin(theta)) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1.0) / sigma;
    if (d > 1.0 - eps) {
      const double sigma2 = sigma * sigma;
      w[0] = 0.5 * dR[0]; w[1] = 0.5 * dR[1]; w[2] = 0.5 * dR[2];
      A = ((sigma - 1.0) * S.s + 1.0) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1.0) * S.s) / (sigma2 * sigma);
    } else {
      theta = acos(d);
      const double k = theta / (2.0 * sqrt(1.0 - d * d));
      w[0] = k * dR[0]; w[1] = k * dR[1]; w[2] = k * dR[2];
      const double theta2 = theta * theta;
      const double a = S.s * sin(theta);
      const double b = S.s * cos(theta);
      const double c = theta2 + sigma * sigma;
      A = (a * sigma + (1.0 - b) * theta) / (theta * c);
      B = (C - ((b - 1.0) * sigma + a * theta) / c) * 1.0 / theta2;
    }
  }
  double Om[9], BOm[9], Om2[9], W[9];
  ess_skew(w, Om);
#pragma unroll
  for (int k = 0; k < 9; k++) BOm[k] = B * Om[k];
  g2o_mul3(BOm, Om, Om2);
#pragma unroll
  for (int k = 0; k < 9; k++) W[k] = (A * Om[k] + Om2[k]) + C * (k % 4 == 0 ? 1.0 : 0.0);
  double u[3] = {S.t[0], S.t[1], S.t[2]};
  ess_solve3<1>(W, u);  // upsilon = W.lu().solve(t)
  br.smallSigma = fabs(sigma) < eps;
  br.smallTheta = d > 1.0 - eps;
  br.theta = theta; br.A = A; br.B = B; br.C = C;
#pragma unroll
  for (int k = 0; k < 9; k++) { br.W[k] = W[k]; br.R[k] = R[k]; }
  out[0] = w[0]; out[1] = w[1]; out[2] = w[2];
  out[3] = u[0]; out[4] = u[1]; out[5] = u[2];
  out[6] = sigma;
}
ORBFE_HD inline void essgraph_log(const OptSim3& S, double out[7]) {
  EssLogBranch br;
  essgraph_log_ex(S, out, br);
}

// the measurement of an edge (src/Optimizer.cc:927-929, :957-959 and the like): Sji = Sjw * Swi
ORBFE_HD inline void ess_measurement(const OptSim3& Siw, const OptSim3& Sjw, OptSim3* Sji) {
  OptSim3 Swi;
  optsim3_inverse(Siw, &Swi);
  optsim3_mul(Sjw, Swi, Sji);
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114) and chi2 with identity information
ORBFE_HD inline double ess_edge_error_ex(const OptSim3& C, const OptSim3& Si, const OptSim3& Sj, double e[7], EssLogBranch& br, OptSim3& E) {
  OptSim3 Sjinv, CSi;
  optsim3_inverse(Sj, &Sjinv);
  optsim3_mul(C, Si, &CSi);
  optsim3_mul(CSi, Sjinv, &E);
  essgraph_log_ex(E, e, br);
  double c = 0.0;
#pragma unroll
  for (int k = 0; k < 7; k++) c = c + e[k] * e[k];
  return c;
}

ORBFE_HD inline double ess_edge_error(const OptSim3& C, const OptSim3& Si, const OptSim3& Sj, double e[7]) {
  EssLogBranch br;
  OptSim3 E;
  return ess_edge_error_ex(C, Si, Sj, e, br, E);
}

// G = d f(E Sim3(xi)) / d xi at xi = 0 of f = Sim3::log as essgraph_log computes it, in the block shape
// [[P, 0, 0], [Q, S, r], [0, 0, 1]] (3 x 3 blocks and a column; order omega, upsilon, sigma).  E Sim3(xi) =
// (R (I + xi_w^), t + s R xi_u, s e^xi_s) to first order, so
//   d omega = P xi_w:  P = (tr(R) I - R^T) / 2 where omega = deltaR(R) / 2 (d > 1 - eps), else the right Jacobian inverse of
//             SO(3), I + Omega / 2 + (1 / theta^2 - (1 + cos theta) / (2 theta sin theta)) Omega^2;
//   d sigma = xi_s;
//   d upsilon = W^-1 (s R xi_u - dW upsilon),  W = A Omega + B Omega^2 + C I,
//             dW upsilon = K d omega + (A_s Omega u + B_s Omega^2 u + C_s u) xi_s,
//             K = -A u^ - B ((Omega u)^ + Omega u^) + (A_t Omega u + B_t Omega^2 u) omega^T / theta.
// A_t, B_t (by theta) and A_s, B_s, C_s (by sigma, ds / d sigma = s) are those of the branch's own formulas: 0 by sigma for
// |sigma| < eps, 0 by theta for d > 1 - eps, and for sigma >= eps, d > 1 - eps those of B = (sigma^2 / 2 - sigma + 1) s / sigma^3
// as sim3.h:199 writes it.
ORBFE_HD inline void ess_log_jacobian(const OptSim3& E, const double e[7], const EssLogBranch& br, double P[9], double Q[9], double S[9],
                                      double r[3]) {
  const double w[3] = {e[0], e[1], e[2]}, u[3] = {e[3], e[4], e[5]}, sigma = e[6], s = E.s, theta = br.theta;
  const double A = br.A, B = br.B;
  double Om[9], Om2[9], ux[9];
  ess_skew(w, Om);
  g2o_mul3(Om, Om, Om2);
  ess_skew(u, ux);
  if (br.smallTheta) {
    const double tr = (br.R[0] + br.R[4]) + br.R[8];
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
      for (int cc = 0; cc < 3; cc++) P[3 * rr + cc] = 0.5 * ((rr == cc ? tr : 0.0) - br.R[3 * cc + rr]);
  } else {
    const double k = 1.0 / (theta * theta) - (1.0 + cos(theta)) / (2.0 * theta * sin(theta));
#pragma unroll
    for (int i = 0; i < 9; i++) P[i] = ((i % 4 == 0 ? 1.0 : 0.0) + 0.5 * Om[i]) + k * Om2[i];
  }
  double At = 0.0, Bt = 0.0, As = 0.0, Bs = 0.0, Cs = 0.0;
  if (!br.smallSigma) Cs = s / sigma - (s - 1.0) / (sigma * sigma);
  if (br.smallSigma && !br.smallTheta) {
    const double t2 = theta * theta, t3 = t2 * theta;
    At = sin(theta) / t2 - 2.0 * (1.0 - cos(theta)) / t3;
    Bt = (1.0 - cos(theta)) / t3 - 3.0 * (theta - sin(theta)) / (t3 * theta);
  } else if (!br.smallSigma && br.smallTheta) {
    As = s / sigma - 2.0 * A / sigma;
    Bs = 0.5 * s / sigma - 3.0 * B / sigma;
  } else if (!br.smallSigma) {
    const double a = s * sin(theta), b = s * cos(theta), t2 = theta * theta, c = t2 + sigma * sigma, DA = theta * c;
    At = ((b * sigma + a * theta + (1.0 - b)) - A * (c + 2.0 * t2)) / DA;
    As = ((a * sigma + a - b * theta) - A * 2.0 * theta * sigma) / DA;
    const double M = (b - 1.0) * sigma + a * theta, Qm = M / c;
    const double Qt = ((-a * sigma + b * theta + a) - Qm * 2.0 * theta) / c;
    const double Qs = ((b * sigma + (b - 1.0) + a * theta) - Qm * 2.0 * sigma) / c;
    Bt = -Qt / t2 - 2.0 * B / theta;
    Bs = (Cs - Qs) / t2;
  }
  double ou[3], o2u[3], oux[9], Oux[9], K[9], KP[9];
  ess_mulv3(Om, u, ou);
  ess_mulv3(Om, ou, o2u);
  ess_skew(ou, oux);
  g2o_mul3(Om, ux, Oux);
#pragma unroll
  for (int i = 0; i < 9; i++) K[i] = -A * ux[i] - B * (oux[i] + Oux[i]);
  if (!br.smallTheta) {
#pragma unroll
    for (int rr = 0; rr < 3; rr++)
#pragma unroll
      for (int cc = 0; cc < 3; cc++) K[3 * rr + cc] = K[3 * rr + cc] + ((At * ou[rr] + Bt * o2u[rr]) * w[cc]) / theta;
  }
  g2o_mul3(K, P, KP);
  // W^-1 [ -K P | s R | -(A_s Omega u + B_s Omega^2 u + C_s u) ]
  double X[21];
#pragma unroll
  for (int rr = 0; rr < 3; rr++) {
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      X[7 * rr + cc] = -KP[3 * rr + cc];
      X[7 * rr + 3 + cc] = s * br.R[3 * rr + cc];
    }
    X[7 * rr + 6] = -((As * ou[rr] + Bs * o2u[rr]) + Cs * u[rr]);
  }
  ess_solve3<7>(br.W, X);
#pragma unroll
  for (int rr = 0; rr < 3; rr++) {
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      Q[3 * rr + cc] = X[7 * rr + cc];
      S[3 * rr + cc] = X[7 * rr + 3 + cc];
    }
    r[rr] = X[7 * rr + 6];
  }
}

// the linearisation of one edge at (Si, Sj): e, J_i = d e / d update_i, J_j (row-major 7 x 7, written straight to Ji / Jj);
// returns chi2.  fixScale: column 6 of both is exactly 0 (oplusImpl zeroes update[6])
ORBFE_HD inline double ess_linearise_edge(const OptSim3& C, const OptSim3& Si, const OptSim3& Sj, bool fixScale, double e[7], double* Ji,
                                          double* Jj) {
  EssLogBranch br;
  OptSim3 E;
  const double chi2 = ess_edge_error_ex(C, Si, Sj, e, br, E);
  double P[9], Q[9], S[9], r[3];
  ess_log_jacobian(E, e, br, P, Q, S, r);
  // S_j <- Sim3(d) S_j gives E Sim3(-d): J_j = -G;  S_i <- Sim3(d) S_i gives E Sim3(Ad(T) d): J_i = G Ad(T),
  // T = S_j S_i^-1 and Ad(T) = [[R, 0, 0], [t^ R, s R, -t], [0, 0, 1]]
  OptSim3 Siinv, T;
  optsim3_inverse(Si, &Siinv);
  optsim3_mul(Sj, Siinv, &T);
  double R[9], tx[9], txR[9], PR[9], QR[9], StxR[9], SR[9], St[3];
  g2o_quat_to_R(T.q, R);
  ess_skew(T.t, tx);
  g2o_mul3(tx, R, txR);
  g2o_mul3(P, R, PR);
  g2o_mul3(Q, R, QR);
  g2o_mul3(S, txR, StxR);
  g2o_mul3(S, R, SR);
  ess_mulv3(S, T.t, St);
  const double k6 = fixScale ? 0.0 : 1.0;
#pragma unroll
  for (int rr = 0; rr < 3; rr++) {
#pragma unroll
    for (int cc = 0; cc < 3; cc++) {
      Ji[7 * rr + cc] = PR[3 * rr + cc];
      Ji[7 * rr + 3 + cc] = 0.0;
      Ji[7 * (rr + 3) + cc] = QR[3 * rr + cc] + StxR[3 * rr + cc];
      Ji[7 * (rr + 3) + 3 + cc] = T.s * SR[3 * rr + cc];
      Jj[7 * rr + cc] = -P[3 * rr + cc];
      Jj[7 * rr + 3 + cc] = 0.0;
      Jj[7 * (rr + 3) + cc] = -Q[3 * rr + cc];
      Jj[7 * (rr + 3) + 3 + cc] = -S[3 * rr + cc];
    }
    Ji[7 * rr + 6] = 0.0;
    Ji[7 * (rr + 3) + 6] = k6 * (r[rr] - St[rr]);
    Jj[7 * rr + 6] = 0.0;
    Jj[7 * (rr + 3) + 6] = k6 * -r[rr];
  }
#pragma unroll
  for (int cc = 0; cc < 6; cc++) { Ji[42 + cc] = 0.0; Jj[42 + cc] = 0.0; }
  Ji[48] = k6;
  Jj[48] = -k6;
  return chi2;
}

// ---------------------------------------------------------------------------------------------------------------------
// Work items
ORBFE_HD inline const double* ess_est_at(const EssArgs& a, int buf, int v) { return a.est + ((size_t)buf * a.nVertices + v) * 8; }
ORBFE_HD inline double* ess_est_at_w(const EssArgs& a, int buf, int v) { return a.est + ((size_t)buf * a.nVertices + v) * 8; }

// once per call, edge e: the measurement, and chi2 at the inputs (what an edge between two fixed vertices keeps)
ORBFE_HD inline void ess_measure_edge(const EssArgs& a, int e) {
  const int i = a.edgeI[e], j = a.edgeJ[e];
  const double* src = a.edgeKind[e] ? a.sim3 : a.sim3Meas;
  OptSim3 Si, Sj, C;
  ess_load(src + 8 * (size_t)i, &Si);
  ess_load(src + 8 * (size_t)j, &Sj);
  ess_measurement(Si, Sj, &C);
  ess_store(C, a.meas + 8 * (size_t)e);
  ess_load(a.sim3 + 8 * (size_t)i, &Si);
  ess_load(a.sim3 + 8 * (size_t)j, &Sj);
  double err[7];
  a.chi2[e] = ess_edge_error(C, Si, Sj, err);
}

// per iteration, active edge k: e, J_i, J_j and chi2 at the estimate `cur`
ORBFE_HD inline void ess_linearise_item(const EssArgs& a, int k, int cur) {
  const int e = a.activeEdge[k];
  OptSim3 Si, Sj, C;
  ess_load(ess_est_at(a, cur, a.edgeI[e]), &Si);
  ess_load(ess_est_at(a, cur, a.edgeJ[e]), &Sj);
  ess_load(a.meas + 8 * (size_t)e, &C);
  double* lin = a.lin + (size_t)kEssLin * e;
  double err[7];
  a.chi2[e] = ess_linearise_edge(C, Si, Sj, a.fixScale != 0, err, lin + 7, lin + 56);
#pragma unroll
  for (int c = 0; c < 7; c++) lin[c] = err[c];
}

// per iteration, item t (a block of H that has edges), lane l: lanes 0 .. 48 own an element of the block, on a diagonal
// block lanes 49 .. 55 an element of b = -sum J^T e.  The edges of the item in ascending order, the seven products of an
// edge in row order: one owner and one order per sum
ORBFE_HD inline void ess_assemble_lane(const EssArgs& a, int t, int lane) {
  const int p = a.itemBlock[t];
  const int col = a.blockCol[p], row = a.rowidx[p];
  const int vr = a.freeVertex[row], vc = a.freeVertex[col];
  const int e0 = a.itemOff[t], e1 = a.itemOff[t + 1];
  if (lane < 49) {
    const int r = lane / 7, c = lane % 7;
    double s = 0.0;
    for (int k = e0; k < e1; k++) {
      const int e = a.itemEdge[k];
      const double* lin = a.lin + (size_t)kEssLin * e;
      const double* Jr = lin + (a.edgeI[e] == vr ? 7 : 56);
      const double* Jc = lin + (a.edgeI[e] == vc ? 7 : 56);
      double d = 0.0;
#pragma unroll
      for (int m = 0; m < 7; m++) d = d + Jr[7 * m + r] * Jc[7 * m + c];
      s = s + d;
    }
    a.H[49 * (size_t)p + lane] = s;
  } else if (lane < 56 && row == col) {
    const int r = lane - 49;
    double s = 0.0;
    for (int k = e0; k < e1; k++) {
      const int e = a.itemEdge[k];
      const double* lin = a.lin + (size_t)kEssLin * e;
      const double* J = lin + (a.edgeI[e] == vr ? 7 : 56);
      double d = 0.0;
#pragma unroll
      for (int m = 0; m < 7; m++) d = d + J[7 * m + r] * lin[m];
      s = s + d;
    }
    a.b[7 * (size_t)row + r] = -s;
  }
}

// per trial, element i of [0, 49 blocksL): L = H + lambda I;  element i of [0, 7 nFree): x = b
ORBFE_HD inline void ess_load_element(const EssArgs& a, size_t i, double lambda) {
  const size_t p = i / 49;
  const int el = (int)(i - 49 * p);
  double v = a.H[i];
  if (a.rowidx[p] == a.blockCol[p] && el % 8 == 0) v = v + lambda;
  a.L[i] = v;
  if (i < 7 * (size_t)a.nFree) a.x[i] = a.b[i];
}

// ---- the block-sparse Cholesky: element operations on L (block-CSC lower triangle, 7 x 7 row-major blocks) ----
// step 1 of column j: element el of block p = (i, j) takes L_ik L_jk^T of every earlier column k that has both, k ascending
ORBFE_HD inline void ess_chol_update_element(const int32_t* updOff, const int32_t* updSrc, double* L, int p, int el) {
  const int r = el / 7, c = el % 7;
  double v = L[49 * (size_t)p + el];
  for (int u = updOff[p]; u < updOff[p + 1]; u++) {
    const double* A = L + 49 * (size_t)updSrc[2 * u] + 7 * r;
    const double* B = L + 49 * (size_t)updSrc[2 * u + 1] + 7 * c;
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 7; m++) s = s + A[m] * B[m];
    v = v - s;
  }
  L[49 * (size_t)p + el] = v;
}
// step 2: the diagonal block in place (lower triangle).  false on a pivot that is not positive (or NaN); the arithmetic runs
// on regardless, so that the caller's loop stays uniform
ORBFE_HD inline bool ess_chol_diag(double* D) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 7; j++) {
    double d = D[8 * j];
#pragma unroll
    for (int m = 0; m < j; m++) d = d - D[7 * j + m] * D[7 * j + m];
    if (!(d > 0.0)) ok = false;
    d = sqrt(d);
    D[8 * j] = d;
#pragma unroll
    for (int i = j + 1; i < 7; i++) {
      double s = D[7 * i + j];
#pragma unroll
      for (int m = 0; m < j; m++) s = s - D[7 * i + m] * D[7 * j + m];
      D[7 * i + j] = s / d;
    }
  }
  return ok;
}
// step 3: row r of an off-diagonal block B of the column: B <- B D^-T
ORBFE_HD inline void ess_chol_scale_row(const double* D, double* B, int r) {
  double* x = B + 7 * r;
#pragma unroll
  for (int c = 0; c < 7; c++) {
    double s = x[c];
#pragma unroll
    for (int m = 0; m < c; m++) s = s - x[m] * D[7 * c + m];
    x[c] = s / D[8 * c];
  }
}
// forward substitution, column j: y_j <- D^-1 y_j, then row r of y_i -= L_ij y_j for every off-diagonal block of the column
ORBFE_HD inline void ess_fwd_diag(const double* D, double* y) {
#pragma unroll
  for (int r = 0; r < 7; r++) {
    double s = y[r];
#pragma unroll
    for (int m = 0; m < r; m++) s = s - D[7 * r + m] * y[m];
    y[r] = s / D[8 * r];
  }
}
ORBFE_HD inline void ess_fwd_row(const double* B, const double* yj, double* yi, int r) {
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < 7; m++) s = s + B[7 * r + m] * yj[m];
  yi[r] = yi[r] - s;
}
// backward substitution, column j: component c of y_j -= sum over the column's off-diagonal blocks (ascending row) of
// L_ij^T x_i, then x_j = D^-T y_j
ORBFE_HD inline void ess_bwd_component(const int32_t* colptr, const int32_t* rowidx, const double* L, double* x, int j, int c) {
  double v = x[7 * (size_t)j + c];
  for (int p = colptr[j] + 1; p < colptr[j + 1]; p++) {
    const double* B = L + 49 * (size_t)p;
    const double* xi = x + 7 * (size_t)rowidx[p];
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < 7; m++) s = s + B[7 * m + c] * xi[m];
    v = v - s;
  }
  x[7 * (size_t)j + c] = v;
}
ORBFE_HD inline void ess_bwd_diag(const double* D, double* y) {
#pragma unroll
  for (int c = 6; c >= 0; c--) {
    double s = y[c];
#pragma unroll
    for (int m = c + 1; m < 7; m++) s = s - D[7 * m + c] * y[m];
    y[c] = s / D[8 * c];
  }
}

// per trial, free vertex f: the trial estimate Sim3(x_f) * S (oplusImpl: x[6] = 0 with fixScale, written into the
// solver's own x, which computeScale reads afterwards)
ORBFE_HD inline void ess_trial_vertex(const EssArgs& a, int f, int cur) {
  double* x = a.x + 7 * (size_t)f;
  if (a.fixScale) x[6] = 0.0;
  const double u[7] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6]};
  const int v = a.freeVertex[f];
  OptSim3 up, S, out;
  optsim3_exp(u, &up);
  ess_load(ess_est_at(a, cur, v), &S);
  optsim3_mul(up, S, &out);
  ess_store(out, ess_est_at_w(a, 1 - cur, v));
}
// per trial, active edge k: chi2 at the trial
ORBFE_HD inline void ess_trial_edge(const EssArgs& a, int k, int cur) {
  const int e = a.activeEdge[k];
  OptSim3 Si, Sj, C;
  ess_load(ess_est_at(a, 1 - cur, a.edgeI[e]), &Si);
  ess_load(ess_est_at(a, 1 - cur, a.edgeJ[e]), &Sj);
  ess_load(a.meas + 8 * (size_t)e, &C);
  double err[7];
  a.chi2[e] = ess_edge_error(C, Si, Sj, err);
}
// the record's partial sums of lane l: chi2 over the active edges, computeScale's sum x . (lambda x + b) over the free
// components, both lane-strided; the caller combines the 64 lanes with the __shfl_down tree 32 .. 1
ORBFE_HD inline void ess_record_lane(const EssArgs& a, int lane, double lambda, double* chi2, double* scale) {
  double c = 0.0, s = 0.0;
  for (int k = lane; k < a.nActive; k += kEssLanes) c = c + a.chi2[a.activeEdge[k]];
  const int n7 = 7 * a.nFree;
  for (int k = lane; k < n7; k += kEssLanes) s = s + a.x[k] * (lambda * a.x[k] + a.b[k]);
  *chi2 = c;
  *scale = s;
}

// iteration 0 takes the user's lambda instead of computeLambdaInit (optimization_algorithm_levenberg.cpp:77-81, :166-168)
ORBFE_HD inline void ess_lm_after_linearise(LbaLM* lm, const LbaRecord& r) {
  lm->cur = r.chi2; lm->ini = r.chi2;
  if (lm->it == 0) { lm->lam = kEssLambdaInit; lm->ni = 2.0; lm->nBad = 0; }
  lm->rho = 0.0; lm->q = 0;
}

// the tail (src/Optimizer.cc:1059-1067): Tiw = [R | t / s] as floats, row-major 4 x 4
ORBFE_HD inline void ess_Tiw(const double* rec8, float* T) {
  OptSim3 S;
  ess_load(rec8, &S);
  double R[9];
  g2o_quat_to_R(S.q, R);
  const double k = 1.0 / S.s;
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
    T[4 * r + 3] = (float)(S.t[r] * k);
  }
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}
// (:1092-1100): P <- Sout[r]^-1 .map( S[r] .map(P) ), in double, stored as float
ORBFE_HD inline void ess_correct_point(const double* Srw8, const double* Sout8, const float P[3], float out[3]) {
  OptSim3 Srw, Sout, Swr;
  ess_load(Srw8, &Srw);
  ess_load(Sout8, &Sout);
  optsim3_inverse(Sout, &Swr);
  const double X[3] = {(double)P[0], (double)P[1], (double)P[2]};
  double Y[3], Z[3];
  optsim3_map(Srw, X, Y);
  optsim3_map(Swr, Y, Z);
  out[0] = (float)Z[0]; out[1] = (float)Z[1]; out[2] = (float)Z[2];
}

}  // namespace orbfe
