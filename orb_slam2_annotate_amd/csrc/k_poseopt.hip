// k_poseopt.hip -- Optimizer::PoseOptimization (src/Optimizer.cc:256-473) as ONE launch: the four rounds, their Levenberg
// iterations and the lambda trials of every iteration run inside k_pose_optimize, one problem per workgroup.  Only the graph
// PoseOptimization builds is covered: one free VertexSE3Expmap, unary EdgeSE3ProjectXYZOnlyPose /
// EdgeStereoSE3ProjectXYZOnlyPose edges, Huber kernel, a dense 6 x 6 system.  All arithmetic is binary64, as in g2o; the
// build has -ffp-contract=off, so every product and sum below rounds where it is written.
//
// Layout.  Lane t of the T = 256 lanes owns edges t, t + T, ...: it alone reads and writes their level and stored chi2.  A
// pass over the edges evaluates them at the pose broadcast in LDS -- a FULL pass at the estimate (error, chi2, Huber weight,
// Jacobian; 21 + 6 + 1 sums) or a TRIAL pass at a trial pose (robust chi2 only).  Summation order, a function of (n, T)
// only: each lane adds its edges in ascending order; the 64 lanes of a wave combine by __shfl_down with offsets 32, 16, 8,
// 4, 2, 1; the four wave sums are added in wave order.  Lane 0 then plays OptimizationAlgorithmLevenberg::solve on the
// 6 x 6 system and broadcasts the next pose and the next command.  Mono edges are carried as three-row edges whose third
// row is zero, and edges outside the active set add +0.0: neither changes a sum.
#include <hip/hip_runtime.h>

#include <cfloat>

#include "kernels.h"
#include "poseopt_kernels.h"

namespace orbfe {
namespace {

constexpr int kT = kPoseOptThreads;
constexpr int kWaves = kT / 64;
constexpr int kSums = 28;  // 21 upper-triangle entries of H (row-major), 6 of b, the robust chi2
enum { CMD_DONE = 0, CMD_FULL = 1, CMD_TRIAL = 2 };

struct Pose { double q[4] /* x y z w */, t[3]; };
struct Cam { double fx, fy, cx, cy, bf, deltaMono, deltaStereo; };

// Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h: quaternionbase_assign_impl<Other, 3, 3>)
__device__ void quat_from_R(const double m[3][3], double q[4]) {
  double t = m[0][0] + m[1][1] + m[2][2];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > (i == 0 ? m[0][0] : m[1][1])) i = 2;
    // j = (i + 1) % 3, k = (j + 1) % 3, written out so that every index is a constant
    if (i == 0) {
      t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
      q[0] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[2][1] - m[1][2]) * t;
      q[1] = (m[1][0] + m[0][1]) * t;
      q[2] = (m[2][0] + m[0][2]) * t;
    } else if (i == 1) {
      t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
      q[1] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[0][2] - m[2][0]) * t;
      q[2] = (m[2][1] + m[1][2]) * t;
      q[0] = (m[0][1] + m[1][0]) * t;
    } else {
      t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
      q[2] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[1][0] - m[0][1]) * t;
      q[0] = (m[0][2] + m[2][0]) * t;
      q[1] = (m[1][2] + m[2][1]) * t;
    }
  }
}

// SE3Quat::normalizeRotation (Thirdparty/g2o/g2o/types/se3quat.h:280-285)
__device__ void normalize_rotation(double q[4]) {
  if (q[3] < 0)
    for (int i = 0; i < 4; i++) q[i] = -q[i];
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] = q[i] / n;
}

// Eigen QuaternionBase::_transformVector: uv = 2 (q.vec x v); v + w uv + q.vec x uv
__device__ __forceinline__ void quat_rotate(const double q[4], double X, double Y, double Z, double* rx, double* ry, double* rz) {
  double uvx = q[1] * Z - q[2] * Y;
  double uvy = q[2] * X - q[0] * Z;
  double uvz = q[0] * Y - q[1] * X;
  uvx = uvx + uvx;
  uvy = uvy + uvy;
  uvz = uvz + uvz;
  *rx = (X + q[3] * uvx) + (q[1] * uvz - q[2] * uvy);
  *ry = (Y + q[3] * uvy) + (q[2] * uvx - q[0] * uvz);
  *rz = (Z + q[3] * uvz) + (q[0] * uvy - q[1] * uvx);
}

// Eigen QuaternionBase::toRotationMatrix
__device__ void quat_to_R(const double q[4], double R[3][3]) {
  const double x = q[0], y = q[1], z = q[2], w = q[3];
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0][0] = 1.0 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
  R[1][0] = txy + twz; R[1][1] = 1.0 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1.0 - (txx + tyy);
}

// VertexSE3Expmap::oplusImpl: SE3Quat::exp(x) * est (se3quat.h:223-257 with its theta < 1e-5 branch, operator* :104-110);
// pow(theta, 3) is taken as theta * theta * theta
__device__ void exp_times(const double x[6], const Pose& est, Pose* out) {
  const double wx = x[0], wy = x[1], wz = x[2];
  const double theta = sqrt(wx * wx + wy * wy + wz * wz);
  const double Om[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
  double Om2[3][3], R[3][3], V[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) Om2[r][c] = (Om[r][0] * Om[0][c] + Om[r][1] * Om[1][c]) + Om[r][2] * Om[2][c];
  if (theta < 0.00001) {
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        R[r][c] = ((r == c ? 1.0 : 0.0) + Om[r][c]) + Om2[r][c];
        V[r][c] = R[r][c];
      }
  } else {
    const double a = sin(theta) / theta;
    const double b = (1.0 - cos(theta)) / (theta * theta);
    const double c3 = (theta - sin(theta)) / (theta * theta * theta);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) {
        const double I = r == c ? 1.0 : 0.0;
        R[r][c] = (I + a * Om[r][c]) + b * Om2[r][c];
        V[r][c] = (I + b * Om[r][c]) + c3 * Om2[r][c];
      }
  }
  double te[3], qe[4];
#pragma unroll
  for (int r = 0; r < 3; r++) te[r] = (V[r][0] * x[3] + V[r][1] * x[4]) + V[r][2] * x[5];
  quat_from_R(R, qe);
  normalize_rotation(qe);  // SE3Quat(Quaterniond, Vector3d)
  double rx, ry, rz;
  quat_rotate(qe, est.t[0], est.t[1], est.t[2], &rx, &ry, &rz);
  out->t[0] = te[0] + rx; out->t[1] = te[1] + ry; out->t[2] = te[2] + rz;
  const double ax = qe[0], ay = qe[1], az = qe[2], aw = qe[3];
  const double bx = est.q[0], by = est.q[1], bz = est.q[2], bw = est.q[3];
  out->q[0] = aw * bx + ax * bw + ay * bz - az * by;
  out->q[1] = aw * by + ay * bw + az * bx - ax * bz;
  out->q[2] = aw * bz + az * bw + ax * by - ay * bx;
  out->q[3] = aw * bw - ax * bx - ay * by - az * bz;
  normalize_rotation(out->q);
}

// (H + lam I) x = b by unpivoted LDL^T; Hs: the 21 upper-triangle entries, row-major.  false on a pivot that is not positive
__device__ bool solve_ldlt(const double* Hs, double lam, const double* b, double x[6]) {
  double A[6][6], L[6][6], D[6], y[6];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = r; c < 6; c++) { A[r][c] = Hs[k]; A[c][r] = Hs[k]; k++; }
#pragma unroll
  for (int j = 0; j < 6; j++) A[j][j] = A[j][j] + lam;
#pragma unroll
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
#pragma unroll
    for (int m = 0; m < j; m++) d = d - (L[j][m] * L[j][m]) * D[m];
    if (!(d > 0.0)) {
#pragma unroll
      for (int i = 0; i < 6; i++) x[i] = 0.0;
      return false;
    }
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; i++) {
      double s = A[j][i];
#pragma unroll
      for (int m = 0; m < j; m++) s = s - (L[i][m] * L[j][m]) * D[m];
      L[i][j] = s / d;
    }
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double s = b[i];
#pragma unroll
    for (int m = 0; m < i; m++) s = s - L[i][m] * y[m];
    y[i] = s;
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double s = y[i] / D[i];
#pragma unroll
    for (int m = i + 1; m < 6; m++) s = s - L[m][i] * x[m];
    x[i] = s;
  }
  return true;
}

struct EdgeConst { double X, Y, Z, u, v, ur, w; };

// computeError + chi2 of one edge at P.  Mono: obs - (x / z * fx + cx, y / z * fy + cy) (types_six_dof_expmap.cpp:290-296);
// stereo: cam_project with its FLOAT invz = 1.0f / z (:299-306).  chi2 = e . (invSigma2 I) e.
__device__ __forceinline__ double edge_error(const Pose& P, const Cam& C, const EdgeConst& E, double e[3], double xyz[3]) {
  double rx, ry, rz;
  quat_rotate(P.q, E.X, E.Y, E.Z, &rx, &ry, &rz);
  const double x = rx + P.t[0], y = ry + P.t[1], z = rz + P.t[2];  // SE3Quat::map (se3quat.h:217-220)
  xyz[0] = x; xyz[1] = y; xyz[2] = z;
  if (E.ur < 0) {  // mvuRight[i] < 0: a monocular edge (src/Optimizer.cc:307)
    e[0] = E.u - ((x / z) * C.fx + C.cx);
    e[1] = E.v - ((y / z) * C.fy + C.cy);
    e[2] = 0.0;
  } else {
    const double invz = (double)(float)(1.0 / z);
    const double p0 = (x * invz) * C.fx + C.cx;
    const double p1 = (y * invz) * C.fy + C.cy;
    const double p2 = p0 - C.bf * invz;
    e[0] = E.u - p0;
    e[1] = E.v - p1;
    e[2] = E.ur - p2;
  }
  return (e[0] * (E.w * e[0]) + e[1] * (E.w * e[1])) + e[2] * (E.w * e[2]);
}

// the sums of the workgroup in the fixed order of the header comment; out[k] valid for every lane on return
template <int K>
__device__ __forceinline__ void block_sum(double (&acc)[K], double* sPart, double* out, int t) {
  const int lane = t & 63, wave = t >> 6;
#pragma unroll
  for (int k = 0; k < K; k++) {
    double v = acc[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
    if (lane == 0) sPart[wave * K + k] = v;
  }
  __syncthreads();
  if (t < K) {
    double s = sPart[t];
    for (int w = 1; w < kWaves; w++) s = s + sPart[w * K + t];
    out[t] = s;
  }
  __syncthreads();
}

template <bool kLds>
__global__ __launch_bounds__(kPoseOptThreads) void k_pose_optimize(PoseOptArgs a) {
  constexpr int kCap = kLds ? kPoseOptLdsEdges : 1;
  __shared__ float sE[7][kCap];
  __shared__ double sPart[kWaves * kSums];
  __shared__ double sSum[kSums];  // H, b, chi2 of the last FULL pass
  __shared__ double sChi[1];      // robust chi2 of the last TRIAL pass / outlier count of a classification
  __shared__ Pose sPose;          // the pose the next pass evaluates
  __shared__ int sCmd;
  __shared__ int sWaveCnt[kWaves];

  const int t = threadIdx.x;
  const PoseOptProblem pr = a.prob[blockIdx.x];
  PoseOptResult* res = a.res + blockIdx.x;
  float4* eA = a.edgeA + pr.off;
  float4* eB = a.edgeB + pr.off;
  uint8_t* level = a.level + pr.off;
  double* chi2s = a.chi2 + pr.off;
  int n = pr.n;

  if (a.gather) {
    // the edges of the table form, in feature order: a feature with a match whose slot is not bad (Optimizer.cc:298-304)
    int base = 0;
    for (int c0 = 0; c0 < pr.n; c0 += kT) {
      const int i = c0 + t;
      int s = -1;
      if (i < pr.n) {
        const int m = a.match[i];
        if (m >= 0) {
          s = a.slot[m];
          if (a.table.flags[s] & ORBFE_MP_BAD) s = -1;
        }
      }
      const unsigned long long mask = __ballot(s >= 0);
      const int lane = t & 63, wave = t >> 6;
      if (lane == 0) sWaveCnt[wave] = __popcll(mask);
      __syncthreads();
      int before = 0, total = 0;
      for (int w = 0; w < kWaves; w++) {
        if (w < wave) before += sWaveCnt[w];
        total += sWaveCnt[w];
      }
      if (s >= 0) {
        const int e = base + before + __popcll(mask & ((1ull << lane) - 1ull));
        const float4 r0 = a.table.rec[2 * (size_t)s];
        eA[e] = make_float4(r0.x, r0.y, r0.z, a.invLevelSigma2[a.featOctave[i]]);
        eB[e] = make_float4(a.featX[i], a.featY[i], a.featUr ? a.featUr[i] : -1.0f, 0.0f);
        a.edgeFeat[e] = i;
      }
      base += total;
      __syncthreads();
    }
    n = base;
    __threadfence_block();
    __syncthreads();
  }

  if (n < 3) {  // nInitialCorrespondences < 3: nothing is touched (Optimizer.cc:385)
    if (t == 0) {
      res->nInliers = 0; res->nEdges = n; res->rounds = 0; res->pad = 0;
      for (int r = 0; r < 4; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
      for (int k = 0; k < 16; k++) res->Tcw[k] = pr.Tcw[k];
    }
    return;
  }

  if (kLds) {
    for (int e = t; e < n; e += kT) {
      const float4 A = eA[e], B = eB[e];
      sE[0][e] = A.x; sE[1][e] = A.y; sE[2][e] = A.z; sE[3][e] = B.x; sE[4][e] = B.y; sE[5][e] = B.z; sE[6][e] = A.w;
    }
  }
  for (int e = t; e < n; e += kT) level[e] = 0;
  __syncthreads();

  auto load = [&](int e, EdgeConst* E) {
    if (kLds) {
      E->X = (double)sE[0][e]; E->Y = (double)sE[1][e]; E->Z = (double)sE[2][e];
      E->u = (double)sE[3][e]; E->v = (double)sE[4][e]; E->ur = (double)sE[5][e]; E->w = (double)sE[6][e];
    } else {
      const float4 A = eA[e], B = eB[e];
      E->X = (double)A.x; E->Y = (double)A.y; E->Z = (double)A.z;
      E->u = (double)B.x; E->v = (double)B.y; E->ur = (double)B.z; E->w = (double)A.w;
    }
  };

  Cam C;
  C.fx = (double)pr.K5[0]; C.fy = (double)pr.K5[1]; C.cx = (double)pr.K5[2]; C.cy = (double)pr.K5[3]; C.bf = (double)pr.K5[4];
  C.deltaMono = (double)a.deltaMono; C.deltaStereo = (double)a.deltaStereo;
  const float thrMono = 5.991f, thrStereo = 7.815f;  // chi2Mono / chi2Stereo (Optimizer.cc:391-392)

  // lane 0's Levenberg state
  Pose start, est;
  double lam = 0.0, ni = 2.0, cur = 0.0, ini = 0.0, x[6] = {0, 0, 0, 0, 0, 0};
  int nBadLM = 0, q = 0, it = 0, iters = 0, trials = 0, nActive = n, nBad = 0, rounds = 0;
  bool ok = true;
  if (t == 0) {  // Converter::toSE3Quat (src/Converter.cc:37-47)
    double R[3][3];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[r][c] = (double)pr.Tcw[4 * r + c];
      start.t[r] = (double)pr.Tcw[4 * r + 3];
    }
    quat_from_R(R, start.q);
    normalize_rotation(start.q);
  }

  for (int rnd = 0; rnd < 4; rnd++) {
    const bool robust = rnd < 3;  // after round index 2 every edge loses its kernel (Optimizer.cc:429-430, :458-459)
    if (t == 0) {
      est = start;  // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) (:399)
      sPose = est;
      sCmd = nActive > 0 ? CMD_FULL : CMD_DONE;  // no active edge: optimize() returns at once (sparse_optimizer.cpp:356)
      it = iters = trials = 0;
      lam = cur = 0.0;
    }
    __syncthreads();
    while (true) {
      const int cmd = sCmd;
      if (cmd == CMD_DONE) break;
      const Pose P = sPose;
      if (cmd == CMD_FULL) {
        // computeActiveErrors + activeRobustChi2 + buildSystem (optimization_algorithm_levenberg.cpp:75-87)
        double acc[kSums];
#pragma unroll
        for (int k = 0; k < kSums; k++) acc[k] = 0.0;
        for (int e = t; e < n; e += kT) {
          if (level[e] != 0) continue;
          EdgeConst E;
          load(e, &E);
          double er[3], p[3];
          const double chi2 = edge_error(P, C, E, er, p);
          chi2s[e] = chi2;
          const bool stereo = !(E.ur < 0);
          const double delta = stereo ? C.deltaStereo : C.deltaMono, dsqr = delta * delta;
          double rho0 = chi2, rho1 = 1.0;
          if (robust && chi2 > dsqr) {  // RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-91)
            const double sq = sqrt(chi2);
            rho0 = 2 * sq * delta - dsqr;
            rho1 = delta / sq;
          }
          // linearizeOplus (types_six_dof_expmap.cpp:266-288, :335-364)
          const double px = p[0], py = p[1];
          const double invz = 1.0 / p[2], invz_2 = invz * invz;
          double J[3][6];
          J[0][0] = px * py * invz_2 * C.fx;
          J[0][1] = -(1.0 + (px * px * invz_2)) * C.fx;
          J[0][2] = py * invz * C.fx;
          J[0][3] = -invz * C.fx;
          J[0][4] = 0.0;
          J[0][5] = px * invz_2 * C.fx;
          J[1][0] = (1.0 + py * py * invz_2) * C.fy;
          J[1][1] = -px * py * invz_2 * C.fy;
          J[1][2] = -px * invz * C.fy;
          J[1][3] = 0.0;
          J[1][4] = -invz * C.fy;
          J[1][5] = py * invz_2 * C.fy;
          if (stereo) {
            J[2][0] = J[0][0] - C.bf * py * invz_2;
            J[2][1] = J[0][1] + C.bf * px * invz_2;
            J[2][2] = J[0][2];
            J[2][3] = J[0][3];
            J[2][4] = 0.0;
            J[2][5] = J[0][5] - C.bf * invz_2;
          } else {
#pragma unroll
            for (int j = 0; j < 6; j++) J[2][j] = 0.0;
          }
          // constructQuadraticForm (base_unary_edge.hpp:43-72): b -= rho1 J^T Omega e, H += J^T (rho1 Omega) J
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
        }
        block_sum<kSums>(acc, sPart, sSum, t);
        if (t == 0) {
          for (int j = 0; j < 6; j++) sSum[21 + j] = -sSum[21 + j];
          cur = ini = sSum[27];
          if (it == 0) {  // computeLambdaInit: tau * max |H_jj| (:166-180)
            double mx = 0.0;
            mx = fmax(fabs(sSum[0]), mx); mx = fmax(fabs(sSum[6]), mx); mx = fmax(fabs(sSum[11]), mx);
            mx = fmax(fabs(sSum[15]), mx); mx = fmax(fabs(sSum[18]), mx); mx = fmax(fabs(sSum[20]), mx);
            lam = 1e-5 * mx;
            ni = 2.0;
            nBadLM = 0;
          }
          q = 0;
          ok = solve_ldlt(sSum, lam, sSum + 21, x);
          Pose trial;
          exp_times(x, est, &trial);
          sPose = trial;
          sCmd = CMD_TRIAL;
        }
      } else {
        // computeActiveErrors + activeRobustChi2 at the trial (:123-124)
        double acc[1] = {0.0};
        for (int e = t; e < n; e += kT) {
          if (level[e] != 0) continue;
          EdgeConst E;
          load(e, &E);
          double er[3], p[3];
          const double chi2 = edge_error(P, C, E, er, p);
          chi2s[e] = chi2;
          const double delta = (E.ur < 0) ? C.deltaMono : C.deltaStereo, dsqr = delta * delta;
          double rho0 = chi2;
          if (robust && chi2 > dsqr) rho0 = 2 * sqrt(chi2) * delta - dsqr;
          acc[0] = acc[0] + rho0;
        }
        block_sum<1>(acc, sPart, sChi, t);
        if (t == 0) {
          double temp = sChi[0];
          if (!ok) temp = DBL_MAX;  // (:126-127)
          const double* b = sSum + 21;
          double scale = 0.0;  // computeScale (:182-189)
          for (int j = 0; j < 6; j++) scale = scale + x[j] * (lam * x[j] + b[j]);
          scale = scale + 1e-3;
          const double rho = (cur - temp) / scale;
          trials++;
          if (rho > 0 && isfinite(temp)) {  // (:134-147)
            const double tt = 2 * rho - 1;
            const double alpha = fmin(1.0 - tt * tt * tt, 2.0 / 3.0);
            lam = lam * fmax(1.0 / 3.0, alpha);
            ni = 2.0;
            cur = temp;
            est = sPose;
          } else {
            lam = lam * ni;
            ni = ni * 2;
          }
          q++;
          if (rho < 0 && q < 10) {  // (:149)
            ok = solve_ldlt(sSum, lam, b, x);
            Pose trial;
            exp_times(x, est, &trial);
            sPose = trial;
            sCmd = CMD_TRIAL;
          } else {
            iters++;
            it++;
            bool stop = (q == 10 || rho == 0);  // (:151-152)
            if (!stop) {
              if ((ini - cur) * 1e3 < ini) nBadLM++;  // Stop criterium (Raul) (:154-161)
              else nBadLM = 0;
              stop = nBadLM >= 3;
            }
            sPose = est;
            sCmd = (stop || it == 10) ? CMD_DONE : CMD_FULL;
          }
        }
      }
      __syncthreads();
    }
    // classification (Optimizer.cc:403-463): an outlier edge is recomputed at the estimate, an inlier keeps the error of the
    // last evaluated trial -- rejected or not
    const Pose P = sPose;
    double cnt[1] = {0.0};
    for (int e = t; e < n; e += kT) {
      EdgeConst E;
      load(e, &E);
      double c2;
      if (level[e] != 0) {
        double er[3], p[3];
        c2 = edge_error(P, C, E, er, p);
        chi2s[e] = c2;
      } else {
        c2 = chi2s[e];
      }
      const bool bad = (float)c2 > ((E.ur < 0) ? thrMono : thrStereo);  // (a NaN chi2 is an inlier)
      level[e] = bad ? 1 : 0;
      cnt[0] = cnt[0] + (bad ? 1.0 : 0.0);
    }
    block_sum<1>(cnt, sPart, sChi, t);
    if (t == 0) {
      nBad = (int)sChi[0];
      nActive = n - nBad;
      res->iterations[rnd] = iters; res->trials[rnd] = trials; res->lambda[rnd] = lam; res->chi2[rnd] = cur;
      rounds = rnd + 1;
    }
    __syncthreads();
    if (n < 10) break;  // optimizer.edges().size() < 10 (:462)
  }

  if (t == 0) {  // Converter::toCvMat (src/Converter.cc:49-71)
    for (int r = rounds; r < 4; r++) { res->iterations[r] = 0; res->trials[r] = 0; res->lambda[r] = 0.0; res->chi2[r] = 0.0; }
    res->nInliers = n - nBad; res->nEdges = n; res->rounds = rounds; res->pad = 0;
    double R[3][3];
    quat_to_R(est.q, R);
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) res->Tcw[4 * r + c] = (float)R[r][c];
      res->Tcw[4 * r + 3] = (float)est.t[r];
    }
    res->Tcw[12] = 0.0f; res->Tcw[13] = 0.0f; res->Tcw[14] = 0.0f; res->Tcw[15] = 1.0f;
  }
}

}  // namespace

void launch_pose_optimize(hipStream_t s, const PoseOptArgs& a, int nProblems, bool lds) {
  if (nProblems <= 0) return;
  if (lds) hipLaunchKernelGGL(k_pose_optimize<true>, dim3(nProblems), dim3(kPoseOptThreads), 0, s, a);
  else hipLaunchKernelGGL(k_pose_optimize<false>, dim3(nProblems), dim3(kPoseOptThreads), 0, s, a);
}

}  // namespace orbfe
