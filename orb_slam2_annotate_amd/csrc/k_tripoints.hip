// k_tripoints.hip -- the kernels of orbfe_create_triangulated_points (include/orbfe.h; host side: tripoints.hip; the
// arithmetic: triangulate_math.h per pair, tripoints_host.h for who is created and for normal and range).  References:
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:283-501), MapPoint::ComputeDistinctiveDescriptors
// (src/MapPoint.cc:269-333) and MapPoint::UpdateNormalAndDepth (:360-404) for a row of two entries.
//
// Two launches on one stream:
//   solve   one lane per pair of the dense list, 256-lane workgroups: tri_pair in registers, exactly as k_triangulate (no
//           LDS, no scratch); position and status go to the dense workspace, an atomicMin on winner[i1] names the first
//           neighbour that succeeds.  The minimum commutes: equal inputs give equal winners
//   place   ONE workgroup of 1024 threads walks the list in chunks of 1024 pairs.  keep = CREATED && winner[i1] == k.  The
//           list is ascending in (k, i1), which is the creation order, so created point number w is the number of kept
//           pairs before it in the list: a ballot per wave, the waves' counts through LDS, a running base across chunks.
//           First walk: the count and the points made per neighbour (an integer sum in LDS: it commutes).  Second walk,
//           only when the count fits `capacity`: point w takes newSlot[w]; position, normal, range, descriptor and flags
//           go straight into the table rows, (k, i1, i2) into the output lists.
// The places never come from arrival order or a counter: equal inputs give equal tables.
#include <hip/hip_runtime.h>

#include "tripoints_host.h"
#include "tripoints_kernels.h"

namespace orbfe {

namespace {

constexpr int kWave = 64, kTpWaves = kTpPlaceThreads / kWave;

__global__ __launch_bounds__(kTpSolveThreads) void k_tri_points_solve(TriPointsArgs a) {
  const TriangulateArgs& A = a.tri;
  const int p = (int)(blockIdx.x * kTpSolveThreads + threadIdx.x);
  if (p >= A.nPairs) return;
  const TriangulatePair P = A.pairs[p];
  const TriCamera c1 = A.cams[0], c2 = A.cams[1 + P.k];
  const TriKeypoint k1 = tri_keypoint(A.frames[0], P.i1, P.depth1, P.xraw1, P.yraw1, A.scaleFactors, A.levelSigma2);
  const TriKeypoint k2 = tri_keypoint(A.frames[1 + P.k], P.i2, P.depth2, P.xraw2, P.yraw2, A.scaleFactors, A.levelSigma2);
  double X[3] = {0.0, 0.0, 0.0};
  const int st = tri_pair(c1, c2, k1, k2, A.ratioFactor, X);
  a.pairStatus[p] = (uint8_t)st;
  if (st == kTriCreated) {
    a.pairPos[p] = make_float4((float)X[0], (float)X[1], (float)X[2], 0.0f);  // the binary64 result rounded once
    atomicMin(&A.winner[P.i1], P.k);
  }
}

// the exclusive prefix of `flag` over the workgroup's threads, on top of *carry, which advances by the chunk's total
__device__ inline int tp_scan_chunk(bool flag, int32_t* waveSum, int* carry) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) waveSum[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kTpWaves; w++) {
    const int c = waveSum[w];
    before += w < wave ? c : 0;
    all += c;
  }
  const int pos = *carry + before + __popcll(mask & ((1ull << lane) - 1ull));
  *carry += all;
  __syncthreads();  // waveSum is rewritten by the next chunk
  return pos;
}

__global__ __launch_bounds__(kTpPlaceThreads) void k_tri_points_place(MapPointsDevice t, TriPointsArgs a) {
  __shared__ int32_t waveSum[kTpWaves];
  __shared__ int32_t perK[kTpMaxNeighbours];
  const TriangulateArgs& A = a.tri;
  const int tid = threadIdx.x, nPairs = A.nPairs;
  if (tid < kTpMaxNeighbours) perK[tid] = 0;
  __syncthreads();

  int created = 0;
  for (int base = 0; base < nPairs; base += kTpPlaceThreads) {
    const int p = base + tid;
    bool keep = false;
    int k = 0;
    if (p < nPairs) {
      const TriangulatePair P = A.pairs[p];
      k = P.k;
      keep = tp_keep(a.pairStatus[p], P.k, A.winner[P.i1]);
    }
    if (keep) atomicAdd(&perK[k], 1);
    (void)tp_scan_chunk(keep, waveSum, &created);
  }
  // (the last chunk's __syncthreads() are behind every atomicAdd)
  if (tid == 0) a.header[0] = created;
  if (tid < kTpMaxNeighbours) a.header[1 + tid] = perK[tid];
  if (created > a.capacity) return;  // (uniform) neither table is touched

  const float top = A.scaleFactors[a.nLevels - 1];
  int w0 = 0;
  for (int base = 0; base < nPairs; base += kTpPlaceThreads) {
    const int p = base + tid;
    bool keep = false;
    TriangulatePair P = {};
    if (p < nPairs) {
      P = A.pairs[p];
      keep = tp_keep(a.pairStatus[p], P.k, A.winner[P.i1]);
    }
    const int w = tp_scan_chunk(keep, waveSum, &w0);
    if (!keep) continue;
    const size_t s = (size_t)a.newSlot[w];
    const TriPointsKeyFrame f1 = a.kfs[0], f2 = a.kfs[1 + P.k];
    const float4 X = a.pairPos[p];
    const float pos[3] = {X.x, X.y, X.z};
    float nrm[3], lo, hi;
    tp_normal_range(pos, f1.ow, f2.ow, f2.first != 0, A.scaleFactors[a.octave1[P.i1]], top, nrm, &lo, &hi);
    t.rec[2 * s] = make_float4(pos[0], pos[1], pos[2], lo);
    t.rec[2 * s + 1] = make_float4(nrm[0], nrm[1], nrm[2], hi);
    // ComputeDistinctiveDescriptors for the row of two: the first entry's descriptor, the key frame with the smaller mnId
    const uint8_t* row = f2.first ? f2.desc + 32 * (size_t)P.i2 : f1.desc + 32 * (size_t)P.i1;
    const uint4* src = reinterpret_cast<const uint4*>(row);
    uint4* dst = reinterpret_cast<uint4*>(t.desc + 32 * s);
    dst[0] = src[0];
    dst[1] = src[1];
    t.flags[s] = (uint8_t)a.flags;
    a.createdK[w] = P.k;
    a.createdI1[w] = P.i1;
    a.createdI2[w] = P.i2;
  }
}

}  // namespace

void launch_tri_points(hipStream_t s, const MapPointsDevice& table, const TriPointsArgs& a) {
  if (a.tri.nPairs <= 0) return;
  const int blocks = (a.tri.nPairs + kTpSolveThreads - 1) / kTpSolveThreads;
  hipLaunchKernelGGL(k_tri_points_solve, dim3(blocks), dim3(kTpSolveThreads), 0, s, a);
  hipLaunchKernelGGL(k_tri_points_place, dim3(1), dim3(kTpPlaceThreads), 0, s, table, a);
}

}  // namespace orbfe
