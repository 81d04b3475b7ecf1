// pnp_math.h -- the arithmetic of PnPsolver (src/PnPsolver.cc:323-354, :401-1083): EPnP on n >= 4 correspondences and the
// per-correspondence test of CheckInliers, written once: k_pnp.hip compiles it for the device, tests/cpp/pnp_cpu.cpp and
// tests/cpp/pnp_host_san.cpp for the host.  Plain C++ without a HIP include.  Arithmetic is binary64 on inputs widened from
// float (build with -ffp-contract=off) and follows the lines cited operation by operation wherever the reference's own
// arithmetic is defined.
//
// Everything of fixed size takes the n-dependent sums as arguments -- the sum of the points (centroid), PW0^T PW0, M^T M, the
// sums of estimate_R_and_t (camera-point centroid, ABt) and the reprojection-error sum -- so that each kernel forms those
// sums in its own fixed order; pnp_compute_pose() below forms them point by point in index order, which is what one lane of
// k_pnp_ransac (n = 4) and the host program do.  All arrays that are indexed at run time live in a PnpWork, which a kernel
// places in LDS: nothing of it goes to scratch.
//
// The OpenCV calls have no arithmetic of their own here (the reference accepts any OpenCV >= 2.4.3).  They are restated:
//   * cvSVD of the symmetric 3 x 3 PW0^T PW0 (:436) and of ABt (:689): jacobi_svd3 of jacobi_math.h (singular values
//     descending).  The sign of a singular-vector pair is free in any SVD, but the control points depend on it, so :436
//     gets a rule: every row of UCt has its component of largest magnitude (the first of equal ones) positive.
//   * cvInvert(CV_SVD) of the 3 x 3 control-point matrix (:473): the pseudo-inverse V diag(1 / w) U^T from jacobi_svd3 with
//     1 / w_i = 0 where w_i <= kPnpSvCut (w_0 + w_1 + w_2), kPnpSvCut = 2 DBL_EPSILON.
//   * cvSolve(CV_SVD) of the 6 x 4, 6 x 3 and 6 x 5 systems (:781, :812, :846): least squares by jacobi_math.h's one-sided
//     iteration on the columns of [A; V], then x = sum_j v_j (a_j . b) / |a_j|^2 over the columns with
//     |a_j| > kPnpSvCut sum_k |a_k|.
//   * cvSVD of the 12 x 12 M^T M for n >= 5 (:561): jacobi_math.h's two-sided iteration; eigenvalues descending, ties by
//     index; ut row 11 is the eigenvector of the smallest one.  NOT bit-identical to cv::SVD.
//   * cvSVD of M^T M for n = 4 (the RANSAC minimal set): M is 8 x 12 and its null space has dimension >= 4, inside which an
//     eigen-solver's basis is rounding noise.  DEVIATION: the basis is canonical instead -- Householder QR of M^T (12 x 8),
//     reflector k maps its column to -sign(alpha) |x| e_1 with sign(0) = +1 (a zero column: no reflector), and ut rows
//     8, 9, 10, 11 are Q e_8 .. Q e_11 with Q = H_1 .. H_8.  One valid instance of what the reference computes (an orthonormal
//     basis of the same subspace) and a continuous function of M wherever M has rank 8.
// qr_solve (:991-1083) is the reference's own Householder loop restated as written; where it returns early on a singular
// column (:1018-1021) the reference leaves X as it was (uninitialised in the first iteration): here X starts as 0.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "jacobi_math.h"  // jacobi_svd3 and both iterations; ORBFE_HD

namespace orbfe {

enum PnpStatus { kPnpOk = 0, kPnpNonfinite = 1 };  // ORBFE_PNP_* of include/orbfe.h

constexpr double kPnpSvCut = 2.0 * DBL_EPSILON;

// fu fv uc vc
struct PnpCamera {
  float fu, fv, uc, vc;
};

// a candidate (one PnPsolver) of a call.  Laid out by pnp_host.h, read by k_pnp.hip.  `hyp0` counts hypotheses in
// k_pnp_ransac and Refine records in k_pnp_refine
struct PnpCandidate {
  int point0, nPoints;  // correspondences [point0, point0 + nPoints) of p3d / p2d / maxErr2
  int hyp0;             // its first hypothesis / record
  int word0, words;     // mask words of its first hypothesis / record; words per hypothesis = ceil(nPoints / 32)
  PnpCamera K;
};

// every array the fixed-size algebra indexes at run time
struct PnpWork {
  double a[144];      // M^T M, both triangles (n >= 5), or M^T as 12 x 8 row-major (n = 4); destroyed
  double v[144];      // the accumulated rotations of pnp_eig12; pnp_null4: the eight reflectors, 12 each
  double ut[4][12];   // ut[i] = ut + 12 * (11 - i) of the reference: v_1 .. v_4 of compute_L_6x10
  double d[12];
  double cws[4][3], ccs[4][3], ci[9];
  double l[60], rho[6];
  double la[30], lv[25], lx[5];          // cvSolve: A (6 x m), V (m x m), x
  double ga[24], gb[6], gx[4], A1[4], A2[4];  // gauss_newton / qr_solve
  double betas[4][4];                    // [1], [2], [3] as the reference
  double Rs[4][9], ts[4][3], err[4];
};

ORBFE_HD inline double pnp_dot3(const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; }  // :621
ORBFE_HD inline double pnp_dist2(const double* p1, const double* p2) {  // :612
  return (p1[0] - p2[0]) * (p1[0] - p2[0]) + (p1[1] - p2[1]) * (p1[1] - p2[1]) + (p1[2] - p2[2]) * (p1[2] - p2[2]);
}

// choose_control_points (:401-445) after its two sums: c0 = the centroid (sum / n, :410), cov = PW0^T PW0 row-major
ORBFE_HD inline void pnp_control_points(const double c0[3], const double cov[9], int n, double cws[4][3]) {
  double U[9], w[3], V[9];
  jacobi_svd3(cov, U, w, V);  // :436: dc = w, uct = U^T
#pragma unroll
  for (int j = 0; j < 3; j++) cws[0][j] = c0[j];
#pragma unroll
  for (int i = 1; i < 4; i++) {
    double r[3] = {U[i - 1], U[3 + i - 1], U[6 + i - 1]};  // row i - 1 of uct
    double big = fabs(r[0]), sg = r[0] < 0.0 ? -1.0 : 1.0;
    if (fabs(r[1]) > big) { big = fabs(r[1]); sg = r[1] < 0.0 ? -1.0 : 1.0; }
    if (fabs(r[2]) > big) { big = fabs(r[2]); sg = r[2] < 0.0 ? -1.0 : 1.0; }
    const double k = sqrt(w[i - 1] / n);  // :441
#pragma unroll
    for (int j = 0; j < 3; j++) cws[i][j] = cws[0][j] + k * (sg * r[j]);  // :443
  }
}

// compute_barycentric_coordinates (:465-473): cc_inv
ORBFE_HD inline void pnp_cc_inv(const double cws[4][3], double ci[9]) {
  double cc[9], U[9], w[3], V[9];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 1; j < 4; j++) cc[3 * i + j - 1] = cws[j][i] - cws[0][i];  // :471
  jacobi_svd3(cc, U, w, V);
  const double cut = kPnpSvCut * (w[0] + w[1] + w[2]);
  double iw[3];
#pragma unroll
  for (int k = 0; k < 3; k++) iw[k] = w[k] > cut ? 1.0 / w[k] : 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++)
      ci[3 * i + j] = V[3 * i] * iw[0] * U[3 * j] + V[3 * i + 1] * iw[1] * U[3 * j + 1] + V[3 * i + 2] * iw[2] * U[3 * j + 2];
}

// :475-485 for one point
ORBFE_HD inline void pnp_alphas(const double ci[9], const double c0[3], const double pw[3], double a[4]) {
#pragma unroll
  for (int j = 0; j < 3; j++)
    a[1 + j] = ci[3 * j] * (pw[0] - c0[0]) + ci[3 * j + 1] * (pw[1] - c0[1]) + ci[3 * j + 2] * (pw[2] - c0[2]);
  a[0] = 1.0 - a[1] - a[2] - a[3];
}

// fill_M (:495-510) for one point: its two rows of M
ORBFE_HD inline void pnp_fill_M(const double as[4], double u, double v, const PnpCamera& K, double M1[12], double M2[12]) {
  const double fu = (double)K.fu, fv = (double)K.fv, uc = (double)K.uc, vc = (double)K.vc;
#pragma unroll
  for (int i = 0; i < 4; i++) {
    M1[3 * i] = as[i] * fu; M1[3 * i + 1] = 0.0; M1[3 * i + 2] = as[i] * (uc - u);
    M2[3 * i] = 0.0; M2[3 * i + 1] = as[i] * fv; M2[3 * i + 2] = as[i] * (vc - v);
  }
}

// the symmetric 12 x 12 W->a -> W->ut: the eigenvectors of the four smallest eigenvalues (see the head of the file)
ORBFE_HD inline void pnp_eig12(PnpWork* W) {
  double* a = W->a;
  double* v = W->v;
  jacobi_identity(v, 12);
  jacobi_sweeps(12, [&](int p, int q) { return jacobi_sym_pair(a, v, 12, p, q); });
  for (int i = 0; i < 12; i++) W->d[i] = a[13 * i];
  // descending, ties by index: the last row is the smallest eigenvalue, of equal ones the one with the highest index
  for (int k = 0; k < 4; k++) {
    int best = -1;
    for (int j = 0; j < 12; j++) {
      if (isnan(W->d[j])) continue;
      if (best < 0 || W->d[j] <= W->d[best]) best = j;
    }
    if (best < 0) best = k;  // (all NaN: any column, the pose is NaN as well)
    for (int r = 0; r < 12; r++) W->ut[k][r] = v[12 * r + best];
    W->d[best] = NAN;
  }
}

// n = 4: W->a holds M^T as 12 x 8 row-major (a[8 i + r] = M[r][i]) -> W->ut (see the head of the file)
ORBFE_HD inline void pnp_null4(PnpWork* W) {
  double* a = W->a;
  double* hv = W->v;  // reflector k: hv[12 k + i], i = k .. 11; hv[12 k + k - 1] unused
  double* vtv = W->d;
  for (int k = 0; k < 8; k++) {
    double s2 = 0.0;
    for (int i = k; i < 12; i++) s2 += a[8 * i + k] * a[8 * i + k];
    const double alpha = a[8 * k + k], nrm = sqrt(s2);
    for (int i = k; i < 12; i++) hv[12 * k + i] = a[8 * i + k];
    hv[12 * k + k] = alpha >= 0.0 ? alpha + nrm : alpha - nrm;  // x - (-sign(alpha) |x|) e_1
    double vv = 0.0;
    for (int i = k; i < 12; i++) vv += hv[12 * k + i] * hv[12 * k + i];
    vtv[k] = vv;
    if (!(vv > 0.0)) continue;  // a zero column (or NaN, which then is in every entry below anyway): H = I
    for (int j = k; j < 8; j++) {
      double w = 0.0;
      for (int i = k; i < 12; i++) w += hv[12 * k + i] * a[8 * i + j];
      const double tau = 2.0 * w / vv;
      for (int i = k; i < 12; i++) a[8 * i + j] = a[8 * i + j] - tau * hv[12 * k + i];
    }
  }
  for (int j = 8; j < 12; j++) {
    double* e = W->ut[11 - j];  // ut row j
    for (int i = 0; i < 12; i++) e[i] = i == j ? 1.0 : 0.0;
    for (int k = 7; k >= 0; k--) {
      if (!(vtv[k] > 0.0)) continue;
      double w = 0.0;
      for (int i = k; i < 12; i++) w += hv[12 * k + i] * e[i];
      const double tau = 2.0 * w / vtv[k];
      for (int i = k; i < 12; i++) e[i] = e[i] - tau * hv[12 * k + i];
    }
  }
}

// compute_L_6x10 (:881-926) and compute_rho (:929-937)
ORBFE_HD inline void pnp_L_and_rho(PnpWork* W) {
  for (int i = 0; i < 6; i++) {
    const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);  // 01 02 03 12 13 23
    double dv[4][3];
    for (int k = 0; k < 4; k++)
#pragma unroll
      for (int c = 0; c < 3; c++) dv[k][c] = W->ut[k][3 * a + c] - W->ut[k][3 * b + c];
    double* row = W->l + 10 * i;
    row[0] = pnp_dot3(dv[0], dv[0]);
    row[1] = 2.0 * pnp_dot3(dv[0], dv[1]);
    row[2] = pnp_dot3(dv[1], dv[1]);
    row[3] = 2.0 * pnp_dot3(dv[0], dv[2]);
    row[4] = 2.0 * pnp_dot3(dv[1], dv[2]);
    row[5] = pnp_dot3(dv[2], dv[2]);
    row[6] = 2.0 * pnp_dot3(dv[0], dv[3]);
    row[7] = 2.0 * pnp_dot3(dv[1], dv[3]);
    row[8] = 2.0 * pnp_dot3(dv[2], dv[3]);
    row[9] = pnp_dot3(dv[3], dv[3]);
    W->rho[i] = pnp_dist2(W->cws[a], W->cws[b]);
  }
}

// cvSolve(L_6xm, Rho, x, CV_SVD): W->la (6 x m row-major) and W->rho -> W->lx (see the head of the file)
ORBFE_HD inline void pnp_ls6(PnpWork* W, int m) {
  double* a = W->la;
  double* v = W->lv;
  const JacobiCols<6> cols = {a, v, m};
  jacobi_identity(v, m);
  jacobi_sweeps(m, [&](int p, int q) { return jacobi_cols_pair(cols, p, q); });
  double* n2 = W->d;  // (free here: pnp_eig12 / pnp_null4 are done with it)
  double sumw = 0.0;
  for (int j = 0; j < m; j++) {
    const double s2 = cols.dot(j, j);
    n2[j] = s2;
    sumw += sqrt(s2);
  }
  const double cut = kPnpSvCut * sumw;
  for (int i = 0; i < m; i++) W->lx[i] = 0.0;
  for (int j = 0; j < m; j++) {
    if (!(sqrt(n2[j]) > cut)) continue;
    double ab = 0.0;
    for (int r = 0; r < 6; r++) ab += a[m * r + j] * W->rho[r];
    const double k = ab / n2[j];
    for (int i = 0; i < m; i++) W->lx[i] += v[m * i + j] * k;
  }
}

// find_betas_approx_1 (:767-794), _2 (:799-826), _3 (:831-858) -> W->betas[1], [2], [3]
ORBFE_HD inline void pnp_find_betas(PnpWork* W, int which) {
  const int m = which == 1 ? 4 : (which == 2 ? 3 : 5);
  for (int i = 0; i < 6; i++)
    for (int j = 0; j < m; j++) W->la[m * i + j] = W->l[10 * i + (which == 1 ? (j < 2 ? j : 3 * (j - 1)) : j)];  // B11 B12 B13 B14
  pnp_ls6(W, m);
  const double* b = W->lx;
  double* betas = W->betas[which];
  if (which == 1) {
    if (b[0] < 0) {
      betas[0] = sqrt(-b[0]); betas[1] = -b[1] / betas[0]; betas[2] = -b[2] / betas[0]; betas[3] = -b[3] / betas[0];
    } else {
      betas[0] = sqrt(b[0]); betas[1] = b[1] / betas[0]; betas[2] = b[2] / betas[0]; betas[3] = b[3] / betas[0];
    }
    return;
  }
  if (b[0] < 0) {
    betas[0] = sqrt(-b[0]);
    betas[1] = (b[2] < 0) ? sqrt(-b[2]) : 0.0;
  } else {
    betas[0] = sqrt(b[0]);
    betas[1] = (b[2] > 0) ? sqrt(b[2]) : 0.0;
  }
  if (b[1] < 0) betas[0] = -betas[0];
  betas[2] = which == 3 ? b[3] / betas[0] : 0.0;
  betas[3] = 0.0;
}

// qr_solve (:991-1083) with nr = 6, nc = 4 on W->ga, W->gb -> W->gx
ORBFE_HD inline void pnp_qr_solve(PnpWork* W) {
  const int nr = 6, nc = 4;
  double* pA = W->ga;
  double* pb = W->gb;
  double* A1 = W->A1;
  double* A2 = W->A2;
  for (int k = 0; k < nc; k++) {
    double eta = fabs(pA[k * nc + k]);
    for (int i = k + 1; i < nr; i++) {  // :1012-1016 as written: the pointer advances after the compare, so the rows that
      const double elt = fabs(pA[(i - 1) * nc + k]);  // are read are k .. nr - 2
      if (eta < elt) eta = elt;
    }
    if (eta == 0) {
      A1[k] = A2[k] = 0.0;
      return;
    }
    double sum = 0.0;
    const double inv_eta = 1. / eta;
    for (int i = k; i < nr; i++) {
      pA[i * nc + k] *= inv_eta;
      sum += pA[i * nc + k] * pA[i * nc + k];
    }
    double sigma = sqrt(sum);
    if (pA[k * nc + k] < 0) sigma = -sigma;
    pA[k * nc + k] += sigma;
    A1[k] = sigma * pA[k * nc + k];
    A2[k] = -eta * sigma;
    for (int j = k + 1; j < nc; j++) {
      double s = 0;
      for (int i = k; i < nr; i++) s += pA[i * nc + k] * pA[i * nc + j];
      const double tau = s / A1[k];
      for (int i = k; i < nr; i++) pA[i * nc + j] -= tau * pA[i * nc + k];
    }
  }
  for (int j = 0; j < nc; j++) {  // b <- Qt b
    double tau = 0;
    for (int i = j; i < nr; i++) tau += pA[i * nc + j] * pb[i];
    tau /= A1[j];
    for (int i = j; i < nr; i++) pb[i] -= tau * pA[i * nc + j];
  }
  double* pX = W->gx;  // X = R-1 b
  pX[nc - 1] = pb[nc - 1] / A2[nc - 1];
  for (int i = nc - 2; i >= 0; i--) {
    double sum = 0;
    for (int j = i + 1; j < nc; j++) sum += pA[i * nc + j] * pX[j];
    pX[i] = (pb[i] - sum) / A2[i];
  }
}

// gauss_newton (:971-989) with compute_A_and_b_gauss_newton (:941-967) on W->betas[which]
ORBFE_HD inline void pnp_gauss_newton(PnpWork* W, int which) {
  double* betas = W->betas[which];
  for (int i = 0; i < 4; i++) W->gx[i] = 0.0;
  for (int k = 0; k < 5; k++) {
    for (int i = 0; i < 6; i++) {
      const double* rowL = W->l + i * 10;
      double* rowA = W->ga + i * 4;
      rowA[0] = 2 * rowL[0] * betas[0] + rowL[1] * betas[1] + rowL[3] * betas[2] + rowL[6] * betas[3];
      rowA[1] = rowL[1] * betas[0] + 2 * rowL[2] * betas[1] + rowL[4] * betas[2] + rowL[7] * betas[3];
      rowA[2] = rowL[3] * betas[0] + rowL[4] * betas[1] + 2 * rowL[5] * betas[2] + rowL[8] * betas[3];
      rowA[3] = rowL[6] * betas[0] + rowL[7] * betas[1] + rowL[8] * betas[2] + 2 * rowL[9] * betas[3];
      W->gb[i] = W->rho[i] - (rowL[0] * betas[0] * betas[0] + rowL[1] * betas[0] * betas[1] + rowL[2] * betas[1] * betas[1] +
                              rowL[3] * betas[0] * betas[2] + rowL[4] * betas[1] * betas[2] + rowL[5] * betas[2] * betas[2] +
                              rowL[6] * betas[0] * betas[3] + rowL[7] * betas[1] * betas[3] + rowL[8] * betas[2] * betas[3] +
                              rowL[9] * betas[3] * betas[3]);
    }
    pnp_qr_solve(W);
    for (int i = 0; i < 4; i++) betas[i] += W->gx[i];
  }
}

// everything between the eigenvectors and the three compute_R_and_t calls (:565-586): W->ut, W->cws -> W->betas
ORBFE_HD inline void pnp_all_betas(PnpWork* W) {
  pnp_L_and_rho(W);
  for (int which = 1; which <= 3; which++) {
    pnp_find_betas(W, which);
    pnp_gauss_newton(W, which);
  }
}

// compute_ccs (:513-525) for W->betas[which]
ORBFE_HD inline void pnp_ccs(PnpWork* W, int which) {
  for (int i = 0; i < 4; i++) W->ccs[i][0] = W->ccs[i][1] = W->ccs[i][2] = 0.0;
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++)
      for (int k = 0; k < 3; k++) W->ccs[j][k] += W->betas[which][i] * W->ut[i][3 * j + k];
}
// compute_pcs (:528-537) for one point
ORBFE_HD inline void pnp_pc(const double a[4], const double ccs[4][3], double pc[3]) {
#pragma unroll
  for (int j = 0; j < 3; j++) pc[j] = a[0] * ccs[0][j] + a[1] * ccs[1][j] + a[2] * ccs[2][j] + a[3] * ccs[3][j];
}
// solve_for_sign (:722-735) on the control points, given pcs of point 0 (every pcs computed afterwards has the sign with it)
ORBFE_HD inline void pnp_solve_for_sign(PnpWork* W, const double pc_first[3]) {
  if (pc_first[2] < 0.0)
    for (int i = 0; i < 4; i++)
      for (int j = 0; j < 3; j++) W->ccs[i][j] = -W->ccs[i][j];
}

// estimate_R_and_t (:648-710) after its sums: pc0, pw0 the centroids (sums / n), abt row-major
ORBFE_HD inline void pnp_estimate_R_and_t(const double pc0[3], const double pw0[3], const double abt[9], double R[9], double t[3]) {
  double U[9], w[3], V[9];
  jacobi_svd3(abt, U, w, V);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) R[3 * i + j] = U[3 * i] * V[3 * j] + U[3 * i + 1] * V[3 * j + 1] + U[3 * i + 2] * V[3 * j + 2];
  const double det = R[0] * R[4] * R[8] + R[1] * R[5] * R[6] + R[2] * R[3] * R[7] - R[2] * R[4] * R[6] - R[1] * R[3] * R[8] -
                     R[0] * R[5] * R[7];
  if (det < 0) { R[6] = -R[6]; R[7] = -R[7]; R[8] = -R[8]; }
  t[0] = pc0[0] - pnp_dot3(R, pw0);
  t[1] = pc0[1] - pnp_dot3(R + 3, pw0);
  t[2] = pc0[2] - pnp_dot3(R + 6, pw0);
}

// one term of reprojection_error (:631-641)
ORBFE_HD inline double pnp_reprojection_term(const double R[9], const double t[3], const PnpCamera& K, const double pw[3], double u,
                                             double v) {
  const double Xc = pnp_dot3(R, pw) + t[0], Yc = pnp_dot3(R + 3, pw) + t[1];
  const double inv_Zc = 1.0 / (pnp_dot3(R + 6, pw) + t[2]);
  const double ue = (double)K.uc + (double)K.fu * Xc * inv_Zc, ve = (double)K.vc + (double)K.fv * Yc * inv_Zc;
  return sqrt((u - ue) * (u - ue) + (v - ve) * (v - ve));
}

// :591-593
ORBFE_HD inline int pnp_choose_N(const double err[4]) {
  int N = 1;
  if (err[2] < err[1]) N = 2;
  if (err[3] < err[N]) N = 3;
  return N;
}

ORBFE_HD inline bool pnp_nonfinite(const double R[9], const double t[3]) {
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 9; i++) ok = ok && isfinite(R[i]);
#pragma unroll
  for (int i = 0; i < 3; i++) ok = ok && isfinite(t[i]);
  return !ok;
}

// CheckInliers (:329-344) for one correspondence, with exactly the reference's mix: Xc, Yc, invZc, distX, distY, error2 are
// float, ue and ve double
ORBFE_HD inline bool pnp_is_inlier(const double R[9], const double t[3], const PnpCamera& K, const float P[3], const float p2d[2],
                                   float maxErr) {
  const float Xc = (float)(R[0] * (double)P[0] + R[1] * (double)P[1] + R[2] * (double)P[2] + t[0]);
  const float Yc = (float)(R[3] * (double)P[0] + R[4] * (double)P[1] + R[5] * (double)P[2] + t[1]);
  const float invZc = (float)(1 / (R[6] * (double)P[0] + R[7] * (double)P[1] + R[8] * (double)P[2] + t[2]));
  const double ue = (double)K.uc + (double)K.fu * (double)Xc * (double)invZc;
  const double ve = (double)K.vc + (double)K.fv * (double)Yc * (double)invZc;
  const float distX = (float)((double)p2d[0] - ue);
  const float distY = (float)((double)p2d[1] - ve);
  const float error2 = distX * distX + distY * distY;
  return error2 < maxErr;
}

// compute_pose (:544-598) with every n-dependent sum formed point by point in index order.  P: n(), get(i, pw, uv) -- the
// i-th correspondence widened to double.  n = 4 takes the canonical null-space basis, n >= 5 the eigenvectors of M^T M.
template <class Pts>
ORBFE_HD inline void pnp_compute_pose(const Pts& P, const PnpCamera& K, PnpWork* W, double R[9], double t[3]) {
  const int n = P.n();
  double pw[3], uv[2], as[4], M1[12], M2[12];
  double sum[3] = {0.0, 0.0, 0.0}, c0[3];
  for (int i = 0; i < n; i++) {
    P.get(i, pw, uv);
    sum[0] += pw[0]; sum[1] += pw[1]; sum[2] += pw[2];
  }
#pragma unroll
  for (int j = 0; j < 3; j++) c0[j] = sum[j] / n;
  double cov[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < n; i++) {
    P.get(i, pw, uv);
    const double d[3] = {pw[0] - c0[0], pw[1] - c0[1], pw[2] - c0[2]};
    cov[0] += d[0] * d[0]; cov[1] += d[0] * d[1]; cov[2] += d[0] * d[2];
    cov[4] += d[1] * d[1]; cov[5] += d[1] * d[2]; cov[8] += d[2] * d[2];
  }
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  pnp_control_points(c0, cov, n, W->cws);
  pnp_cc_inv(W->cws, W->ci);
  if (n == 4) {
    for (int i = 0; i < 4; i++) {
      P.get(i, pw, uv);
      pnp_alphas(W->ci, c0, pw, as);
      pnp_fill_M(as, uv[0], uv[1], K, M1, M2);
      for (int c = 0; c < 12; c++) { W->a[8 * c + 2 * i] = M1[c]; W->a[8 * c + 2 * i + 1] = M2[c]; }
    }
    pnp_null4(W);
  } else {
    for (int i = 0; i < 144; i++) W->a[i] = 0.0;
    for (int i = 0; i < n; i++) {
      P.get(i, pw, uv);
      pnp_alphas(W->ci, c0, pw, as);
      pnp_fill_M(as, uv[0], uv[1], K, M1, M2);
      for (int r = 0; r < 12; r++)
        for (int c = r; c < 12; c++) W->a[12 * r + c] += M1[r] * M1[c] + M2[r] * M2[c];
    }
    for (int r = 0; r < 12; r++)
      for (int c = 0; c < r; c++) W->a[12 * r + c] = W->a[12 * c + r];
    pnp_eig12(W);
  }
  pnp_all_betas(W);
  for (int which = 1; which <= 3; which++) {
    pnp_ccs(W, which);
    double pc[3];
    P.get(0, pw, uv);
    pnp_alphas(W->ci, c0, pw, as);
    pnp_pc(as, W->ccs, pc);
    pnp_solve_for_sign(W, pc);
    double pcs[3] = {0.0, 0.0, 0.0}, pc0[3];
    for (int i = 0; i < n; i++) {
      P.get(i, pw, uv);
      pnp_alphas(W->ci, c0, pw, as);
      pnp_pc(as, W->ccs, pc);
      pcs[0] += pc[0]; pcs[1] += pc[1]; pcs[2] += pc[2];
    }
#pragma unroll
    for (int j = 0; j < 3; j++) pc0[j] = pcs[j] / n;
    double abt[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = 0; i < n; i++) {
      P.get(i, pw, uv);
      pnp_alphas(W->ci, c0, pw, as);
      pnp_pc(as, W->ccs, pc);
#pragma unroll
      for (int j = 0; j < 3; j++) {
        abt[3 * j] += (pc[j] - pc0[j]) * (pw[0] - c0[0]);
        abt[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - c0[1]);
        abt[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - c0[2]);
      }
    }
    double Rn[9], tn[3];
    pnp_estimate_R_and_t(pc0, c0, abt, Rn, tn);
    double e = 0.0;
    for (int i = 0; i < n; i++) {
      P.get(i, pw, uv);
      e += pnp_reprojection_term(Rn, tn, K, pw, uv[0], uv[1]);
    }
    W->err[which] = e / n;
    for (int j = 0; j < 9; j++) W->Rs[which][j] = Rn[j];
    for (int j = 0; j < 3; j++) W->ts[which][j] = tn[j];
  }
  const int N = pnp_choose_N(W->err);
  for (int j = 0; j < 9; j++) R[j] = W->Rs[N][j];
  for (int j = 0; j < 3; j++) t[j] = W->ts[N][j];
}

}  // namespace orbfe
