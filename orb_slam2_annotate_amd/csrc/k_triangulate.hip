// k_triangulate.hip -- the per-pair loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:331-501) as one launch:
// one lane per matched pair of the call's dense pair list, the arithmetic of triangulate_math.h in binary64.  No LDS and no
// scratch: the 4 x 4 Jacobi SVD is fully unrolled on compile-time indices, so A and V live in registers.  Lanes of a wave
// leave the sweep loop together (__all), which changes no lane's result: a converged lane rotates nothing.
#include <hip/hip_runtime.h>

#include "triangulate_kernels.h"

namespace orbfe {

namespace {

__global__ __launch_bounds__(kTriangulateThreads) void k_triangulate(TriangulateArgs A) {
  const int p = (int)(blockIdx.x * kTriangulateThreads + threadIdx.x);
  if (p >= A.nPairs) return;
  const TriangulatePair P = A.pairs[p];
  const TriCamera c1 = A.cams[0], c2 = A.cams[1 + P.k];
  const TriKeypoint k1 = tri_keypoint(A.frames[0], P.i1, P.depth1, P.xraw1, P.yraw1, A.scaleFactors, A.levelSigma2);
  const TriKeypoint k2 = tri_keypoint(A.frames[1 + P.k], P.i2, P.depth2, P.xraw2, P.yraw2, A.scaleFactors, A.levelSigma2);
  double X[3] = {0.0, 0.0, 0.0};
  const int st = tri_pair(c1, c2, k1, k2, A.ratioFactor, X);
  const size_t slot = (size_t)P.k * (size_t)A.n1 + (size_t)P.i1;
  A.status[slot] = (uint8_t)st;
  if (st == kTriCreated) {
    A.x3d[3 * slot] = (float)X[0]; A.x3d[3 * slot + 1] = (float)X[1]; A.x3d[3 * slot + 2] = (float)X[2];
    atomicMin(&A.winner[P.i1], P.k);
    atomicAdd(&A.nCreated[P.k], 1);
  }
}

}  // namespace

void launch_triangulate(hipStream_t s, const TriangulateArgs& a) {
  if (a.nPairs <= 0) return;
  const int blocks = (a.nPairs + kTriangulateThreads - 1) / kTriangulateThreads;
  hipLaunchKernelGGL(k_triangulate, dim3(blocks), dim3(kTriangulateThreads), 0, s, a);
}

}  // namespace orbfe
