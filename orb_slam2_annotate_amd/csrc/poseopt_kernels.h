// poseopt_kernels.h -- argument blocks and launcher of the pose-only optimisation kernel (k_poseopt.hip; host side: poseopt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"
#include "poseopt_math.h"  // PoseOptProblem, PoseOptResult, the constants

namespace orbfe {

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
