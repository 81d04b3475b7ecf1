// triangulate_kernels.h -- argument block and launcher of the triangulation kernel (k_triangulate.hip; host side:
// triangulate.hip).  The per-pair arithmetic is triangulate_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "triangulate_math.h"

namespace orbfe {

constexpr int kTriangulateThreads = 256;  // one lane per matched pair
constexpr int32_t kTriangulateNoWinner = 0x7f7f7f7f;  // winner[] as up_fill(0x7f) leaves it: above every neighbour index

// a frame's keypoint arrays on the device (a resident frame's own, or uploaded with the call)
struct TriangulateFrame {
  const float *x, *y, *ur;  // ur NULL: a monocular frame
  const int32_t* octave;
};

struct TriangulateArgs {
  const TriangulatePair* pairs;
  int nPairs, n1;
  const TriangulateFrame* frames;  // [K + 1]: key frame 1, then the neighbours
  const TriCamera* cams;           // [K + 1], the same order
  const float *scaleFactors, *levelSigma2;
  float ratioFactor;
  float* x3d;          // [K * n1 * 3]
  uint8_t* status;     // [K * n1]
  int32_t* nCreated;   // [K]
  int32_t* winner;     // [n1]
};

void launch_triangulate(hipStream_t s, const TriangulateArgs& a);

// keypoint i of a frame as tri_pair reads it (k_triangulate.hip, k_tripoints.hip)
__device__ inline TriKeypoint tri_keypoint(const TriangulateFrame& f, int i, float depth, float xraw, float yraw,
                                           const float* scaleFactors, const float* levelSigma2) {
  TriKeypoint k;
  k.x = f.x[i]; k.y = f.y[i];
  k.ur = f.ur ? f.ur[i] : -1.0f;
  k.depth = depth; k.xraw = xraw; k.yraw = yraw;
  const int o = f.octave[i];
  k.sigma2 = levelSigma2[o]; k.scale = scaleFactors[o];
  return k;
}

}  // namespace orbfe
