// lba_math.h -- the arithmetic of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:483-814) and Optimizer::BundleAdjustment
// (:54-253), written once: k_lba.hip compiles it for the device, tests/cpp/lba_cpu.cpp for the host.  Plain C++ without a HIP
// include.  It covers the one graph both build -- VertexSE3Expmap key-frame poses (free or fixed), marginalised
// VertexSBAPointXYZ points, an EdgeSE3ProjectXYZ or EdgeStereoSE3ProjectXYZ per observation, Huber kernel, Levenberg on the
// Schur complement of the points -- from
//
// * Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp} (computeError / isDepthPositive .h:94-104, :126-136, linearizeOplus
//   .cpp:103-139, :188-234, cam_project :141-157, VertexSE3Expmap::oplusImpl), types_sba.h (VertexSBAPointXYZ::oplusImpl),
// * Thirdparty/g2o/g2o/types/se3quat.h (exp :223-257, operator* :104-110, map :217-220, normalizeRotation :280-285),
// * Thirdparty/g2o/g2o/core/base_binary_edge.hpp:54-120 (constructQuadraticForm), robust_kernel_impl.cpp:78-91 (Huber),
// * Thirdparty/g2o/g2o/core/block_solver.hpp:354-487 (solve: the Schur complement), :502-590 (buildSystem, setLambda),
// * Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp (optimize, terminate).
//
// Arithmetic is binary64 on inputs widened from float (build with -ffp-contract=off).  The header has three layers: the
// edge / SE3 arithmetic, the WORK ITEMS of the kernels (lba_*_point, lba_*_lane / lba_*_finish: what one thread or one lane
// of a wave does, on the arrays of LbaArgs) and the Levenberg rules (LbaLM) the host drives the passes with.  A wave's sums
// are 64 lane-strided partial sums combined by the __shfl_down tree 32 .. 1; the CPU program combines the same partial sums
// in the same tree, so both give the same bits.
#pragma once
#include "g2o_math.h"

namespace orbfe {

constexpr int kLbaLanes = 64;
constexpr int kLbaLin = 48;        // doubles per edge of LbaArgs::lin: A 21 | g 6 | W 18 | 3 unused
constexpr int kLbaPoseSums = 27;   // a free pose's 21 + 6 sums
constexpr int kLbaBlockSums = 36;  // a 6 x 6 block of the reduced system
constexpr int kLbaMaxTrials = 10;  // _maxTrialsAfterFailure
constexpr double kLbaChi2Mono = 5.991, kLbaChi2Stereo = 7.815;  // src/Optimizer.cc:714, :730

// why a round's optimize() ended
enum { kLbaEndNone = 0, kLbaEndIterations = 1, kLbaEndTrials = 2, kLbaEndRhoZero = 3, kLbaEndNoProgress = 4, kLbaEndStop = 5 };

// what the host reads back after a linearisation (chi2, maxDiag, nActive) and after a trial (chi2, scale, ok)
struct LbaRecord {
  double chi2, scale, maxDiag;
  int32_t ok, nActive;
};

// The arrays of a call.  Poses: local first, then fixed; the free ones (local and not local_is_fixed) have an index f in
// [0, nFree).  Estimates are kept twice, [0] and [1]: one is the estimate, the other the trial of the current Levenberg step.
struct LbaArgs {
  int32_t nPoses, nFree, nPoints, nEdges;
  const float* cam;           // [nPoses][8]: fx fy cx cy bf
  const int32_t* freeOf;      // [nPoses]: f or -1
  const float* edgeObs;       // [nEdges][4]: u v u_right invSigma2
  const int32_t* edgePose;    // [nEdges]
  const int32_t* edgePoint;   // [nEdges], non-decreasing
  const int32_t* ptOff;       // [nPoints + 1]: the edges of point p
  const int32_t* poseOff;     // [nFree + 1]: CSR over poseEdge
  const int32_t* poseEdge;    // the edges of free pose f, ascending
  const int32_t* edgeOf;      // [nFree][nPoints]: the edge of (f, p) or -1
  const int32_t* blockPose;   // [nFree (nFree + 1) / 2][2]: (i1 <= i2) of an upper block of the reduced system
  double* pose;               // [2][nPoses][8]: q (x y z w), t, unused
  double* pt;                 // [2][nPoints][3]
  uint8_t* level;             // [nEdges]
  double* chi2;               // [nEdges]: the chi2 of the last evaluation the edge was active in
  double* lin;                // [nEdges][kLbaLin]
  double* Y;                  // [nEdges][18]: W_e (Hll + lambda I)^-1
  double* Hll;                // [nPoints][6] upper, row-major
  double* bl;                 // [nPoints][3]
  double* HllInv;             // [nPoints][6]
  double* Db;                 // [nPoints][3]: (Hll + lambda I)^-1 b_l
  double* ptRho;              // [nPoints]: robust chi2 of the point's active edges
  double* ptScale;            // [nPoints]: the point's part of computeScale
  uint8_t* ptAct;             // [nPoints]: has an active edge
  double* Hpp;                // [nFree][21] upper, row-major
  double* bp;                 // [nFree][6]
  double* poseScale;          // [nFree]
  uint8_t* poseAct;           // [nFree]
  double* S;                  // [6 nFree][6 nFree]: the reduced system, then its Cholesky factor in the lower triangle
  double* bs;                 // [6 nFree]: bschur, overwritten by the substitutions
  double* xp;                 // [6 nFree]
  LbaRecord* rec;
};

// ---------------------------------------------------------------------------------------------------------------------
// SE3Quat (the quaternion arithmetic is g2o_math.h)
// Converter::toSE3Quat (src/Converter.cc:37-47) of a row-major 4 x 4 float pose into the 8 doubles of LbaArgs::pose
ORBFE_HD inline void lba_pose_from_Tcw(const float* T, double* P) {
  double R[9];
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) R[3 * r + c] = (double)T[4 * r + c];
  g2o_quat_from_R(R, P);
  g2o_normalize_rotation(P);
  P[4] = (double)T[3]; P[5] = (double)T[7]; P[6] = (double)T[11]; P[7] = 0.0;
}
// SE3Quat::to_homogeneous_matrix, row-major 4 x 4
ORBFE_HD inline void lba_pose_to_Tcw(const double* P, double* T) {
  double R[9];
  g2o_quat_to_R(P, R);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = R[3 * r + c];
    T[4 * r + 3] = P[4 + r];
  }
  T[12] = 0.0; T[13] = 0.0; T[14] = 0.0; T[15] = 1.0;
}
// VertexSE3Expmap::oplusImpl: out = SE3Quat::exp(x) * est; x = (omega, upsilon)
ORBFE_HD inline void lba_pose_oplus(const double* est, const double x[6], double* out) {
  g2o_se3_oplus(x, est, out);
  out[7] = 0.0;
}

// ---------------------------------------------------------------------------------------------------------------------
// The two edges.  A monocular edge is carried with a third row of zeros: adding +0.0 changes no sum.
struct LbaEdge {
  double e[3], chi2, w;   // error, e . (w e), invSigma2
  double x, y, z;         // the point in the camera
  bool stereo;
};
// computeError (types_six_dof_expmap.h:94-104, :126-136) with cam_project (.cpp:141-157); z is what isDepthPositive tests
ORBFE_HD inline void lba_edge_error(const double* P, const float* cam, const double* X, const float* obs, LbaEdge* E) {
  const double K[5] = {(double)cam[0], (double)cam[1], (double)cam[2], (double)cam[3], (double)cam[4]};
  double xyz[3];
  E->stereo = !(obs[2] < 0.0f);  // mvuRight < 0: monocular (src/Optimizer.cc:627)
  E->w = (double)obs[3];
  E->chi2 = g2o_se3_project_error(P, K, X, (double)obs[0], (double)obs[1], (double)obs[2], E->w, E->e, xyz);
  E->x = xyz[0]; E->y = xyz[1]; E->z = xyz[2];
}
// linearizeOplus (.cpp:103-139, :188-234): Jp = _jacobianOplusXj [3][6], Jl = _jacobianOplusXi [3][3].  These blocks DIVIDE by
// z and z_2; the pose-only edges of poseopt_math.h multiply by invz and invz_2 (.cpp:266-288, :335-364) and round differently:
// the two Jacobians are not copies and stay apart
ORBFE_HD inline void lba_edge_jacobians(const double* P, const float* cam, const LbaEdge& E, double Jp[18], double Jl[9]) {
  const double fx = (double)cam[0], fy = (double)cam[1], bf = (double)cam[4];
  const double x = E.x, y = E.y, z = E.z, z_2 = z * z;
  double R[9];
  g2o_quat_to_R(P, R);
  Jp[0] = x * y / z_2 * fx; Jp[1] = -(1 + (x * x / z_2)) * fx; Jp[2] = y / z * fx; Jp[3] = -1. / z * fx; Jp[4] = 0.0; Jp[5] = x / z_2 * fx;
  Jp[6] = (1 + y * y / z_2) * fy; Jp[7] = -x * y / z_2 * fy; Jp[8] = -x / z * fy; Jp[9] = 0.0; Jp[10] = -1. / z * fy; Jp[11] = y / z_2 * fy;
  if (E.stereo) {
    for (int c = 0; c < 3; c++) {
      Jl[c] = -fx * R[c] / z + fx * x * R[6 + c] / z_2;
      Jl[3 + c] = -fy * R[3 + c] / z + fy * y * R[6 + c] / z_2;
      Jl[6 + c] = Jl[c] - bf * R[6 + c] / z_2;
    }
    Jp[12] = Jp[0] - bf * y / z_2; Jp[13] = Jp[1] + bf * x / z_2; Jp[14] = Jp[2]; Jp[15] = Jp[3]; Jp[16] = 0.0; Jp[17] = Jp[5] - bf / z_2;
  } else {
    // -1. / z * tmp * R with tmp = [fx 0 -x/z fx; 0 fy -y/z fy]: the scaled tmp first, then the product
    const double s = -1. / z;
    const double a00 = s * fx, a02 = s * (-x / z * fx), a11 = s * fy, a12 = s * (-y / z * fy);
    for (int c = 0; c < 3; c++) {
      Jl[c] = a00 * R[c] + a02 * R[6 + c];
      Jl[3 + c] = a11 * R[3 + c] + a12 * R[6 + c];
      Jl[6 + c] = 0.0;
    }
    for (int k = 12; k < 18; k++) Jp[k] = 0.0;
  }
}

// Matrix3d::inverse() of the symmetric H + lam I (Eigen compute_inverse_size3: cofactors over the determinant); H, inv: 6 upper
ORBFE_HD inline void lba_inv3(const double H[6], double lam, double inv[6]) {
  const double a = H[0] + lam, b = H[1], c = H[2], d = H[3] + lam, e = H[4], f = H[5] + lam;
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double det = (c00 * a + c01 * b) + c02 * c;
  const double invdet = 1.0 / det;
  inv[0] = c00 * invdet; inv[1] = c01 * invdet; inv[2] = c02 * invdet;
  inv[3] = (a * f - c * c) * invdet; inv[4] = (b * c - a * e) * invdet; inv[5] = (a * d - b * b) * invdet;
}
ORBFE_HD inline double lba_sym3(const double M[6], int r, int c) {
  return M[r == 0 ? c : c == 0 ? r : (r == 1 || c == 1) ? (r == 1 && c == 1 ? 3 : 4) : 5];
}

// ---------------------------------------------------------------------------------------------------------------------
// Work items.  `cur` is which of the two estimate buffers holds the estimate.
ORBFE_HD inline const double* lba_pose_at(const LbaArgs& a, int buf, int j) { return a.pose + ((size_t)buf * a.nPoses + j) * 8; }
ORBFE_HD inline double* lba_pt_at(const LbaArgs& a, int buf, int p) { return a.pt + ((size_t)buf * a.nPoints + p) * 3; }
// const float thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815) (src/Optimizer.cc:601-602), widened: literals, so the choice
// is a select between two constants (read from the argument block it was an indexed load from a stack copy)
constexpr double kLbaDeltaMono = 0x1.394ca8p+1, kLbaDeltaStereo = 0x1.65d4p+1;
ORBFE_HD inline double lba_delta(const LbaEdge& E) { return E.stereo ? kLbaDeltaStereo : kLbaDeltaMono; }

// linearise: point p walks its active edges ascending at the estimate (computeActiveErrors + buildSystem): every edge's chi2
// and, for an edge to a free pose, A_e = Jp^T W Jp, g_e = Jp^T W e, W_e = Jp^T W Jl; the point's Hll, b_l, robust chi2
ORBFE_HD inline void lba_linearise_point(const LbaArgs& a, int p, int cur, bool robust) {
  const double* X = lba_pt_at(a, cur, p);
  double H[6] = {0, 0, 0, 0, 0, 0}, b[3] = {0, 0, 0}, rho = 0.0;
  int nAct = 0;
  for (int e = a.ptOff[p]; e < a.ptOff[p + 1]; e++) {
    if (a.level[e] != 0) continue;
    nAct++;
    const int j = a.edgePose[e];
    const double* P = lba_pose_at(a, cur, j);
    LbaEdge E;
    lba_edge_error(P, a.cam + 8 * (size_t)j, X, a.edgeObs + 4 * (size_t)e, &E);
    a.chi2[e] = E.chi2;
    double rho0, rho1;
    g2o_huber(E.chi2, lba_delta(E), robust, &rho0, &rho1);
    rho = rho + rho0;
    double Jp[18], Jl[9];
    lba_edge_jacobians(P, a.cam + 8 * (size_t)j, E, Jp, Jl);
    const double wr = rho1 * E.w;
    const double we[3] = {wr * E.e[0], wr * E.e[1], wr * E.e[2]};
    int k = 0;
    for (int r = 0; r < 3; r++)
      for (int c = r; c < 3; c++, k++)
        H[k] = H[k] + (((Jl[r] * wr) * Jl[c] + (Jl[3 + r] * wr) * Jl[3 + c]) + (Jl[6 + r] * wr) * Jl[6 + c]);
    for (int r = 0; r < 3; r++) b[r] = b[r] - ((Jl[r] * we[0] + Jl[3 + r] * we[1]) + Jl[6 + r] * we[2]);
    if (a.freeOf[j] < 0) continue;  // a fixed vertex has no block: the edge feeds Hll and b_l only
    double* L = a.lin + (size_t)e * kLbaLin;
    k = 0;
    for (int r = 0; r < 6; r++)
      for (int c = r; c < 6; c++, k++) L[k] = ((Jp[r] * wr) * Jp[c] + (Jp[6 + r] * wr) * Jp[6 + c]) + (Jp[12 + r] * wr) * Jp[12 + c];
    for (int r = 0; r < 6; r++) L[21 + r] = (Jp[r] * we[0] + Jp[6 + r] * we[1]) + Jp[12 + r] * we[2];
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 3; c++) L[27 + 3 * r + c] = ((Jp[r] * wr) * Jl[c] + (Jp[6 + r] * wr) * Jl[3 + c]) + (Jp[12 + r] * wr) * Jl[6 + c];
  }
  for (int k = 0; k < 6; k++) a.Hll[6 * (size_t)p + k] = H[k];
  for (int k = 0; k < 3; k++) a.bl[3 * (size_t)p + k] = b[k];
  a.ptRho[p] = rho;
  a.ptScale[p] = 0.0;
  a.ptAct[p] = nAct > 0;
}

// pose blocks: lane `lane` of free pose f's wave adds A_e and g_e of the pose's active edges lane, lane + 64, ... ascending
ORBFE_HD inline void lba_pose_block_lane(const LbaArgs& a, int f, int lane, double acc[kLbaPoseSums], int* nAct) {
  for (int k = 0; k < kLbaPoseSums; k++) acc[k] = 0.0;
  *nAct = 0;
  for (int i = a.poseOff[f] + lane; i < a.poseOff[f + 1]; i += kLbaLanes) {
    const int e = a.poseEdge[i];
    if (a.level[e] != 0) continue;
    *nAct = *nAct + 1;
    const double* L = a.lin + (size_t)e * kLbaLin;
    for (int k = 0; k < kLbaPoseSums; k++) acc[k] = acc[k] + L[k];
  }
}
ORBFE_HD inline void lba_pose_block_finish(const LbaArgs& a, int f, const double tot[kLbaPoseSums], int nAct) {
  for (int k = 0; k < 21; k++) a.Hpp[21 * (size_t)f + k] = tot[k];
  for (int k = 0; k < 6; k++) a.bp[6 * (size_t)f + k] = -tot[21 + k];
  a.poseScale[f] = 0.0;
  a.poseAct[f] = nAct > 0;
}

// Schur, per point and trial: (Hll + lambda I)^-1, Db = that times b_l, and Y_e = W_e (Hll + lambda I)^-1 of its active edges
ORBFE_HD inline void lba_schur_point(const LbaArgs& a, int p, double lambda) {
  if (!a.ptAct[p]) return;
  double inv[6];
  lba_inv3(a.Hll + 6 * (size_t)p, lambda, inv);
  for (int k = 0; k < 6; k++) a.HllInv[6 * (size_t)p + k] = inv[k];
  const double* b = a.bl + 3 * (size_t)p;
  for (int r = 0; r < 3; r++) a.Db[3 * (size_t)p + r] = (lba_sym3(inv, r, 0) * b[0] + lba_sym3(inv, r, 1) * b[1]) + lba_sym3(inv, r, 2) * b[2];
  for (int e = a.ptOff[p]; e < a.ptOff[p + 1]; e++) {
    if (a.level[e] != 0 || a.freeOf[a.edgePose[e]] < 0) continue;
    const double* W = a.lin + (size_t)e * kLbaLin + 27;
    double* Y = a.Y + 18 * (size_t)e;
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 3; c++)
        Y[3 * r + c] = (W[3 * r] * lba_sym3(inv, 0, c) + W[3 * r + 1] * lba_sym3(inv, 1, c)) + W[3 * r + 2] * lba_sym3(inv, 2, c);
  }
}

// Schur, upper block (i1 <= i2): the lane adds Y_e1 W_e2^T over the active edges e1 of pose i1 (lane, lane + 64, ... of its
// list, ascending) whose point pose i2 sees through an active edge e2
ORBFE_HD inline void lba_schur_block_lane(const LbaArgs& a, int i1, int i2, int lane, double acc[kLbaBlockSums]) {
  for (int k = 0; k < kLbaBlockSums; k++) acc[k] = 0.0;
  for (int i = a.poseOff[i1] + lane; i < a.poseOff[i1 + 1]; i += kLbaLanes) {
    const int e1 = a.poseEdge[i];
    if (a.level[e1] != 0) continue;
    const int e2 = i1 == i2 ? e1 : a.edgeOf[(size_t)i2 * a.nPoints + a.edgePoint[e1]];
    if (e2 < 0 || a.level[e2] != 0) continue;
    const double* Y = a.Y + 18 * (size_t)e1;
    const double* W = a.lin + (size_t)e2 * kLbaLin + 27;
    for (int r = 0; r < 6; r++)
      for (int c = 0; c < 6; c++)
        acc[6 * r + c] = acc[6 * r + c] + ((Y[3 * r] * W[3 * c] + Y[3 * r + 1] * W[3 * c + 1]) + Y[3 * r + 2] * W[3 * c + 2]);
  }
}
// Hschur(i1, i2) = [i1 == i2] (Hpp + lambda I) - sum, written to both triangles of S; a pose without an active edge is not
// in the active set: its diagonal block is the identity, so its step is zero
ORBFE_HD inline void lba_schur_block_finish(const LbaArgs& a, int i1, int i2, const double tot[kLbaBlockSums], double lambda) {
  const size_t n = 6 * (size_t)a.nFree;
  for (int r = 0; r < 6; r++)
    for (int c = 0; c < 6; c++) {
      double v;
      if (i1 == i2) {
        const int lo = r < c ? r : c, hi = r < c ? c : r;
        const double h = a.Hpp[21 * (size_t)i1 + (lo * 6 - lo * (lo - 1) / 2) + (hi - lo)];
        v = a.poseAct[i1] ? (r == c ? h + lambda : h) - tot[6 * r + c] : (r == c ? 1.0 : 0.0);
      } else {
        v = 0.0 - tot[6 * r + c];
      }
      a.S[(6 * (size_t)i1 + r) * n + 6 * i2 + c] = v;
      if (i1 != i2) a.S[(6 * (size_t)i2 + c) * n + 6 * i1 + r] = v;
    }
}
// bschur of free pose f: b_p - sum W_e Db(point of e) over the pose's active edges, the same lanes and order
ORBFE_HD inline void lba_schur_rhs_lane(const LbaArgs& a, int f, int lane, double acc[6]) {
  for (int k = 0; k < 6; k++) acc[k] = 0.0;
  for (int i = a.poseOff[f] + lane; i < a.poseOff[f + 1]; i += kLbaLanes) {
    const int e = a.poseEdge[i];
    if (a.level[e] != 0) continue;
    const double* W = a.lin + (size_t)e * kLbaLin + 27;
    const double* D = a.Db + 3 * (size_t)a.edgePoint[e];
    for (int r = 0; r < 6; r++) acc[r] = acc[r] + ((W[3 * r] * D[0] + W[3 * r + 1] * D[1]) + W[3 * r + 2] * D[2]);
  }
}
ORBFE_HD inline void lba_schur_rhs_finish(const LbaArgs& a, int f, const double tot[6]) {
  for (int r = 0; r < 6; r++) a.bs[6 * (size_t)f + r] = a.poseAct[f] ? a.bp[6 * (size_t)f + r] - tot[r] : 0.0;
}

// The dense solve, as element operations: Cholesky L L^T in the lower triangle of S, right-looking, column j at a time, then
// column-oriented substitutions on bs.  Each element has one owner per step, so any split over threads gives the same bits.
ORBFE_HD inline bool lba_chol_pivot(double* S, size_t n, size_t j) {  // false: a non-positive (or NaN) pivot
  const double d = S[j * n + j];
  if (!(d > 0.0)) return false;
  S[j * n + j] = sqrt(d);
  return true;
}
ORBFE_HD inline void lba_chol_scale(double* S, size_t n, size_t j, size_t i) { S[i * n + j] = S[i * n + j] / S[j * n + j]; }
ORBFE_HD inline void lba_chol_update(double* S, size_t n, size_t j, size_t i, size_t k) {  // j < k <= i
  S[i * n + k] = S[i * n + k] - S[i * n + j] * S[k * n + j];
}
// after the solve: the trial of free pose f and its part of computeScale; ok false: the step is zero
ORBFE_HD inline void lba_pose_trial(const LbaArgs& a, int j, int cur, double lambda) {
  const double* est = lba_pose_at(a, cur, j);
  double* out = a.pose + ((size_t)(1 - cur) * a.nPoses + j) * 8;
  const int f = a.freeOf[j];
  if (f < 0 || !a.poseAct[f]) {
    for (int k = 0; k < 8; k++) out[k] = est[k];
    if (f >= 0) a.poseScale[f] = 0.0;
    return;
  }
  const double* x = a.xp + 6 * (size_t)f;
  lba_pose_oplus(est, x, out);
  double s = 0.0;
  for (int k = 0; k < 6; k++) s = s + x[k] * (lambda * x[k] + a.bp[6 * (size_t)f + k]);
  a.poseScale[f] = s;
}

// back-substitution, update and the errors-only pass of point p: x_l = (Hll + lambda I)^-1 (b_l - sum W_e^T x_p), the trial
// point, its part of computeScale; then chi2 of its active edges at the trial (what chi2() reads later) and their robust sum
ORBFE_HD inline void lba_trial_point(const LbaArgs& a, int p, int cur, double lambda, bool robust, bool ok) {
  const double* X = lba_pt_at(a, cur, p);
  double* Xt = lba_pt_at(a, 1 - cur, p);
  if (!a.ptAct[p]) {
    for (int k = 0; k < 3; k++) Xt[k] = X[k];
    a.ptScale[p] = 0.0; a.ptRho[p] = 0.0;
    return;
  }
  const double* b = a.bl + 3 * (size_t)p;
  double c[3] = {b[0], b[1], b[2]}, xl[3] = {0.0, 0.0, 0.0};
  if (ok) {
    for (int e = a.ptOff[p]; e < a.ptOff[p + 1]; e++) {
      const int f = a.freeOf[a.edgePose[e]];
      if (a.level[e] != 0 || f < 0) continue;
      const double* W = a.lin + (size_t)e * kLbaLin + 27;
      const double* x = a.xp + 6 * (size_t)f;
      for (int k = 0; k < 3; k++) {
        double s = W[k] * x[0];
        for (int r = 1; r < 6; r++) s = s + W[3 * r + k] * x[r];
        c[k] = c[k] - s;
      }
    }
    const double* inv = a.HllInv + 6 * (size_t)p;
    for (int r = 0; r < 3; r++) xl[r] = (lba_sym3(inv, r, 0) * c[0] + lba_sym3(inv, r, 1) * c[1]) + lba_sym3(inv, r, 2) * c[2];
  }
  double s = 0.0;
  for (int k = 0; k < 3; k++) {
    Xt[k] = X[k] + xl[k];
    s = s + xl[k] * (lambda * xl[k] + b[k]);
  }
  a.ptScale[p] = s;
  double rho = 0.0;
  for (int e = a.ptOff[p]; e < a.ptOff[p + 1]; e++) {
    if (a.level[e] != 0) continue;
    const int j = a.edgePose[e];
    LbaEdge E;
    lba_edge_error(lba_pose_at(a, 1 - cur, j), a.cam + 8 * (size_t)j, Xt, a.edgeObs + 4 * (size_t)e, &E);
    a.chi2[e] = E.chi2;
    double rho0, rho1;
    g2o_huber(E.chi2, lba_delta(E), robust, &rho0, &rho1);
    rho = rho + rho0;
  }
  a.ptRho[p] = rho;
}

// the record of a pass: one wave; the lane adds the poses' then the points' parts (lane, lane + 64, ... ascending)
struct LbaTotals {
  double chi2, scale, maxDiag;
  int nActive;
};
ORBFE_HD inline void lba_totals_lane(const LbaArgs& a, int lane, LbaTotals* t) {
  t->chi2 = 0.0; t->scale = 0.0; t->maxDiag = 0.0; t->nActive = 0;
  for (int f = lane; f < a.nFree; f += kLbaLanes) {
    if (!a.poseAct[f]) continue;
    t->scale = t->scale + a.poseScale[f];
    for (int r = 0; r < 6; r++) t->maxDiag = fmax(fabs(a.Hpp[21 * (size_t)f + (r * 6 - r * (r - 1) / 2)]), t->maxDiag);
  }
  for (int p = lane; p < a.nPoints; p += kLbaLanes) {
    if (!a.ptAct[p]) continue;
    t->nActive = t->nActive + 1;
    t->chi2 = t->chi2 + a.ptRho[p];
    t->scale = t->scale + a.ptScale[p];
    const double* H = a.Hll + 6 * (size_t)p;
    t->maxDiag = fmax(fmax(fabs(H[0]), fabs(H[3])), fmax(fabs(H[5]), t->maxDiag));
  }
}

// classification of edge e at the estimate `cur` (src/Optimizer.cc:706-736, :749-777): chi2() is what the last pass the
// edge was active in stored, isDepthPositive() is evaluated now.  first: the edge goes to level 1.  final: erase[e] = 0
// kept, 1 erased and level 1, 2 erased by the final test only
ORBFE_HD inline bool lba_edge_bad(const LbaArgs& a, int e, int cur) {
  const int j = a.edgePose[e];
  const double* P = lba_pose_at(a, cur, j);
  const double* X = lba_pt_at(a, cur, a.edgePoint[e]);
  double c[3];
  g2o_quat_rotate(P, X[0], X[1], X[2], c);
  const double z = c[2] + P[6];
  const double thr = a.edgeObs[4 * (size_t)e + 2] < 0.0f ? kLbaChi2Mono : kLbaChi2Stereo;
  return a.chi2[e] > thr || !(z > 0.0);
}

// ---------------------------------------------------------------------------------------------------------------------
// The Levenberg rules of one optimize() call (optimization_algorithm_levenberg.cpp:61-164) around the passes
struct LbaLM {
  double lam, ni, cur, ini, rho;
  int it, q, trials, nBad, maxIt, end;
};
ORBFE_HD inline void lba_lm_begin(LbaLM* lm, int maxIt) {
  lm->lam = 0.0; lm->ni = 2.0; lm->cur = 0.0; lm->ini = 0.0; lm->rho = 0.0;
  lm->it = 0; lm->q = 0; lm->trials = 0; lm->nBad = 0; lm->maxIt = maxIt; lm->end = kLbaEndNone;
}
// after computeActiveErrors + activeRobustChi2 + buildSystem of iteration lm->it
ORBFE_HD inline void lba_lm_after_linearise(LbaLM* lm, const LbaRecord& r) {
  lm->cur = r.chi2; lm->ini = r.chi2;
  if (lm->it == 0) {  // computeLambdaInit: _tau = 1e-5
    lm->lam = 1e-5 * r.maxDiag; lm->ni = 2.0; lm->nBad = 0;
  }
  lm->rho = 0.0; lm->q = 0;
}
// after a trial at lm->lam: true when the trial is accepted (the trial becomes the estimate)
ORBFE_HD inline bool lba_lm_after_trial(LbaLM* lm, const LbaRecord& r) {
  const double temp = r.ok ? r.chi2 : DBL_MAX;
  const double scale = r.scale + 1e-3;
  lm->rho = (lm->cur - temp) / scale;
  lm->trials++;
  lm->q++;
  if (lm->rho > 0 && isfinite(temp)) {
    const double tt = 2 * lm->rho - 1;
    double alpha = 1. - tt * tt * tt;
    alpha = alpha < 2. / 3. ? alpha : 2. / 3.;
    lm->lam = lm->lam * (1. / 3. > alpha ? 1. / 3. : alpha);
    lm->ni = 2.0;
    lm->cur = temp;
    return true;
  }
  lm->lam = lm->lam * lm->ni;
  lm->ni = lm->ni * 2;
  return false;
}
// the do-while condition of the trial loop without terminate()
ORBFE_HD inline bool lba_lm_more_trials(const LbaLM& lm) { return lm.rho < 0 && lm.q < kLbaMaxTrials; }
// after the trial loop: true when optimize() goes on to the next iteration
ORBFE_HD inline bool lba_lm_after_iteration(LbaLM* lm) {
  lm->it++;
  if (lm->q == kLbaMaxTrials) { lm->end = kLbaEndTrials; return false; }
  if (lm->rho == 0) { lm->end = kLbaEndRhoZero; return false; }
  if ((lm->ini - lm->cur) * 1e3 < lm->ini) lm->nBad++;  // Stop criterium (Raul)
  else lm->nBad = 0;
  if (lm->nBad >= 3) { lm->end = kLbaEndNoProgress; return false; }
  if (lm->it >= lm->maxIt) { lm->end = kLbaEndIterations; return false; }
  return true;
}

}  // namespace orbfe
