// poseopt_math.h -- the arithmetic of Optimizer::PoseOptimization (src/Optimizer.cc:256-473), written once: k_poseopt.hip
// compiles it for the device, tests/cpp/poseopt_cpu.cpp for the host.  Plain C++ without a HIP include.  It covers the one
// graph PoseOptimization builds -- one free VertexSE3Expmap, unary EdgeSE3ProjectXYZOnlyPose /
// EdgeStereoSE3ProjectXYZOnlyPose edges, Huber kernel, Levenberg on a dense 6 x 6 system -- from
//
// * Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp (computeError / cam_project :290-306, linearizeOplus :266-288, :335-364),
// * Thirdparty/g2o/g2o/core/base_unary_edge.hpp:43-72 (constructQuadraticForm), src/Converter.cc:37-71,
// * and, through g2o_math.h, se3quat.h, robust_kernel_impl.cpp and optimization_algorithm_levenberg.cpp.
//
// Arithmetic is binary64 on inputs widened from float (build with -ffp-contract=off).  Mono edges are carried as three-row
// edges whose third row is zero: adding +0.0 changes no sum.
#pragma once
#include "g2o_math.h"

namespace orbfe {

constexpr int kPoseOptThreads = 256;   // T: lane t of the workgroup owns edges t, t + T, t + 2T, ...
constexpr int kPoseOptMaxEdges = 16384;  // the frame limit of include/orbfe.h
// Edge constants (Xw, obs, invSigma2: 7 floats = 28 bytes) are staged in LDS for problems of up to this many edges and re-read
// from global memory above it.  A CU has 160 KiB of LDS, of which one workgroup may declare 64 KiB statically: 2048 edges
// take 56 KiB, the reduction scratch and the pose broadcast 2 KiB more, and two problems still share a CU.  ORB-SLAM2 asks
// for at most 2000 features per frame.
constexpr int kPoseOptLdsEdges = 2048;
constexpr int kPoseOptSums = 28;  // 21 upper-triangle entries of H (row-major), 6 of b, the robust chi2
constexpr int kPoseOptMaxIt = 10;  // optimizer.optimize(its[it]), its = {10, 10, 10, 10} (Optimizer.cc:393)
constexpr float kPoseOptChi2Mono = 5.991f, kPoseOptChi2Stereo = 7.815f;  // chi2Mono / chi2Stereo (:391-392)

// One problem of a call.  Array form: edges [off, off + n) of the edge arrays.  Table form: n = features of the frame, the
// kernel makes the edges itself.
struct PoseOptProblem {
  int32_t off, n;
  float K5[5];    // fx fy cx cy bf
  float Tcw[16];  // the start pose (row-major 4 x 4)
  float pad;
};

struct PoseOptResult {
  int32_t nInliers, nEdges, rounds, pad;
  int32_t iterations[4], trials[4];
  double lambda[4], chi2[4];
  float Tcw[16];
};

struct PoseOptPose { double p[7]; };  // q (x y z w), then t: the layout g2o_se3_oplus reads
struct PoseOptCam { double K[5] /* fx fy cx cy bf */, deltaMono, deltaStereo; };
struct PoseOptEdge { double X[3], u, v, ur, w; };

// ur < 0: a monocular edge (mvuRight[i] < 0, src/Optimizer.cc:307)
ORBFE_HD inline double poseopt_delta(const PoseOptCam& C, const PoseOptEdge& E) { return (E.ur < 0) ? C.deltaMono : C.deltaStereo; }

// FULL work item of one active edge at P: error and chi2 (returned: what the edge stores), Huber, Jacobian, and
// constructQuadraticForm (base_unary_edge.hpp:43-72) into the 28 sums: H += J^T (rho1 Omega) J, b += rho1 J^T Omega e
// (negated once, after the sum), chi2 += rho0
ORBFE_HD inline double poseopt_edge_full(const PoseOptPose& P, const PoseOptCam& C, const PoseOptEdge& E, bool robust,
                                         double (&acc)[kPoseOptSums]) {
  double er[3], p[3], rho0, rho1;
  const double chi2 = g2o_se3_project_error(P.p, C.K, E.X, E.u, E.v, E.ur, E.w, er, p);
  g2o_huber(chi2, poseopt_delta(C, E), robust, &rho0, &rho1);
  // linearizeOplus (types_six_dof_expmap.cpp:266-288, :335-364).  These blocks MULTIPLY by invz and invz_2; the binary edges
  // of lba_math.h divide by z and z_2 (.cpp:103-139, :188-234) and round differently: the two Jacobians are not copies
  const double fx = C.K[0], fy = C.K[1], bf = C.K[4];
  const double px = p[0], py = p[1];
  const double invz = 1.0 / p[2], invz_2 = invz * invz;
  double J[3][6];
  J[0][0] = px * py * invz_2 * fx;
  J[0][1] = -(1.0 + (px * px * invz_2)) * fx;
  J[0][2] = py * invz * fx;
  J[0][3] = -invz * fx;
  J[0][4] = 0.0;
  J[0][5] = px * invz_2 * fx;
  J[1][0] = (1.0 + py * py * invz_2) * fy;
  J[1][1] = -px * py * invz_2 * fy;
  J[1][2] = -px * invz * fy;
  J[1][3] = 0.0;
  J[1][4] = -invz * fy;
  J[1][5] = py * invz_2 * fy;
  if (!(E.ur < 0)) {
    J[2][0] = J[0][0] - bf * py * invz_2;
    J[2][1] = J[0][1] + bf * px * invz_2;
    J[2][2] = J[0][2];
    J[2][3] = J[0][3];
    J[2][4] = 0.0;
    J[2][5] = J[0][5] - bf * invz_2;
  } else {
#pragma unroll
    for (int j = 0; j < 6; j++) J[2][j] = 0.0;
  }
  const double wr = rho1 * E.w;
  const double we0 = wr * er[0], we1 = wr * er[1], we2 = wr * er[2];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = r; c < 6; c++) {
      acc[k] = acc[k] + (((J[0][r] * wr) * J[0][c] + (J[1][r] * wr) * J[1][c]) + (J[2][r] * wr) * J[2][c]);
      k++;
    }
#pragma unroll
  for (int j = 0; j < 6; j++) acc[21 + j] = acc[21 + j] + ((J[0][j] * we0 + J[1][j] * we1) + J[2][j] * we2);
  acc[27] = acc[27] + rho0;
  return chi2;
}

// TRIAL work item of one active edge at the trial P: its chi2 (returned) and its robust chi2 onto *sum
ORBFE_HD inline double poseopt_edge_trial(const PoseOptPose& P, const PoseOptCam& C, const PoseOptEdge& E, bool robust, double* sum) {
  double er[3], p[3], rho0, rho1;
  const double chi2 = g2o_se3_project_error(P.p, C.K, E.X, E.u, E.v, E.ur, E.w, er, p);
  g2o_huber(chi2, poseopt_delta(C, E), robust, &rho0, &rho1);
  *sum = *sum + rho0;
  return chi2;
}

// the chi2 an outlier edge is classified on: recomputed at the estimate (Optimizer.cc:403-463)
ORBFE_HD inline double poseopt_edge_chi2(const PoseOptPose& P, const PoseOptCam& C, const PoseOptEdge& E) {
  double er[3], p[3];
  return g2o_se3_project_error(P.p, C.K, E.X, E.u, E.v, E.ur, E.w, er, p);
}

// const float chi2 = e->chi2(); chi2 > chi2Mono[it] / chi2Stereo[it] (:408-414, :424-430): a NaN chi2 is an inlier
ORBFE_HD inline bool poseopt_is_outlier(double c2, const PoseOptEdge& E) {
  return (float)c2 > ((E.ur < 0) ? kPoseOptChi2Mono : kPoseOptChi2Stereo);
}

// Converter::toSE3Quat (src/Converter.cc:37-47) of a row-major 4 x 4 float pose
ORBFE_HD inline void poseopt_pose_from_Tcw(const float T[16], PoseOptPose* P) {
  double R[9];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[3 * r + c] = (double)T[4 * r + c];
    P->p[4 + r] = (double)T[4 * r + 3];
  }
  g2o_quat_from_R(R, P->p);
  g2o_normalize_rotation(P->p);
}

// Converter::toCvMat(SE3Quat) (src/Converter.cc:49-71): to_homogeneous_matrix, double -> float
ORBFE_HD inline void poseopt_pose_to_Tcw(const PoseOptPose& P, float T[16]) {
  double R[9];
  g2o_quat_to_R(P.p, R);
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) T[4 * r + c] = (float)R[3 * r + c];
    T[4 * r + 3] = (float)P.p[4 + r];
  }
  T[12] = 0.0f; T[13] = 0.0f; T[14] = 0.0f; T[15] = 1.0f;
}

// solve (H + lam I) x = b and form the trial SE3Quat::exp(x) * est (VertexSE3Expmap::oplusImpl)
ORBFE_HD inline void poseopt_lm_propose(G2oLM<6>* s, const PoseOptPose& est, PoseOptPose* trial) {
  s->ok = g2o_solve_ldlt<6>(s->S, s->lam, s->S + 21, s->x);
  g2o_se3_oplus(s->x, est.p, trial->p);
}

// what a problem of fewer than 3 edges yields: nothing is touched (nInitialCorrespondences < 3, Optimizer.cc:385)
ORBFE_HD inline void poseopt_result_untouched(const PoseOptProblem& pr, int n, PoseOptResult* res) {
  res->nInliers = 0; res->nEdges = n; res->rounds = 0; res->pad = 0;
  for (int r = 0; r < 4; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
  for (int k = 0; k < 16; k++) res->Tcw[k] = pr.Tcw[k];
}

}  // namespace orbfe
