// poseopt_kernels.h -- argument blocks and launcher of the pose-only optimisation kernel (k_poseopt.hip; host side: poseopt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"

namespace orbfe {

constexpr int kPoseOptThreads = 256;   // T: lane t of the workgroup owns edges t, t + T, t + 2T, ...
constexpr int kPoseOptMaxEdges = 16384;  // the frame limit of include/orbfe.h
// Edge constants (Xw, obs, invSigma2: 7 floats = 28 bytes) are staged in LDS for problems of up to this many edges and re-read
// from global memory above it.  A CU has 160 KiB of LDS, of which one workgroup may declare 64 KiB statically: 2048 edges
// take 56 KiB, the reduction scratch and the pose broadcast 2 KiB more, and two problems still share a CU.  ORB-SLAM2 asks
// for at most 2000 features per frame.
constexpr int kPoseOptLdsEdges = 2048;

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

struct PoseOptArgs {
  const PoseOptProblem* prob;
  PoseOptResult* res;
  float4* edgeA;   // (Xw.x, Xw.y, Xw.z, invSigma2) per edge
  float4* edgeB;   // (u, v, u_right, 0)
  uint8_t* level;  // per edge: 0 inlier, 1 outlier (the result flags)
  double* chi2;    // per edge: chi2 of the error g2o would hold (the classification chi2 on return)
  float deltaMono, deltaStereo;  // (float)sqrt(5.991), (float)sqrt(7.815) (src/Optimizer.cc:291-292)
  // table form (gather != 0): one problem; edge e is the e-th feature i with match[i] >= 0 whose slot is not bad
  int gather;
  MapPointsDevice table;
  const int32_t* slot;
  const int32_t* match;
  const float *featX, *featY, *featUr;  // featUr NULL: a monocular frame
  const int32_t* featOctave;
  const float* invLevelSigma2;
  int32_t* edgeFeat;  // [n] feature index of edge e
};

// one workgroup per problem; lds: every problem of the call has at most kPoseOptLdsEdges edges (features, in the table form)
void launch_pose_optimize(hipStream_t s, const PoseOptArgs& a, int nProblems, bool lds);

}  // namespace orbfe
