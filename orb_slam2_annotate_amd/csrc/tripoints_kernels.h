// tripoints_kernels.h -- launch interface of k_tripoints.hip (host side: tripoints.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "match_kernels.h"
#include "triangulate_kernels.h"

namespace orbfe {

constexpr int kTpSolveThreads = 256;   // one lane per pair, as k_triangulate
constexpr int kTpPlaceThreads = 1024;  // one workgroup walks the pair list in chunks of this many pairs
constexpr int kTpMaxNeighbours = 64;   // kTriHostMaxNeighbours: the per-neighbour counts live in LDS

// what the placing kernel reads of a key frame besides its keypoints: entry 0 is key frame 1, entry 1 + k neighbour k
struct TriPointsKeyFrame {
  const uint8_t* desc;  // the resident frame's descriptor rows
  float ow[3];          // the centre the graph's mirror holds for the kf slot
  int32_t first;        // neighbours only: 1 when its mnId is below key frame 1's (it stands first in the row of two)
};

// One orbfe_create_triangulated_points call.  tri: the operands of the per-pair solve (x3d / status / nCreated unused: the
// solve writes the dense arrays below; winner [n1] starts as kTriangulateNoWinner).  pairPos [nPairs] (x, y, z, unused) and
// pairStatus [nPairs] are indexed like tri.pairs.  header [1 + kTpMaxNeighbours]: created, then the points made per
// neighbour.  createdK / createdI1 / createdI2 [min(capacity, nPairs)] and the table rows are written only when created <=
// capacity; newSlot [min(capacity, nPairs)]; scale [nLevels] is tri.scaleFactors.
struct TriPointsArgs {
  TriangulateArgs tri;
  const TriPointsKeyFrame* kfs;  // [K + 1]
  const int32_t* octave1;        // key frame 1's octaves
  int nLevels, capacity, flags;
  float4* pairPos;
  uint8_t* pairStatus;
  const int32_t* newSlot;
  int32_t *header, *createdK, *createdI1, *createdI2;
};
void launch_tri_points(hipStream_t s, const MapPointsDevice& table, const TriPointsArgs& a);

}  // namespace orbfe
