// k_obsdesc.hip -- MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) over the rows of the device
// observation graph and the key frames' descriptors the handle holds (include/orbfe.h:
// orbfe_obsgraph_distinctive_descriptors*; host side: obsdesc.hip).
//
// One wave per point, nothing but registers: lane j holds entry j of the row and its key frame's 32 descriptor bytes in 8
// VGPRs.  For every live entry i, in row order, descriptor i is broadcast by v_readlane, every lane computes d[i][j], and
// the (size_t)(0.5 * (N - 1))-th smallest of the N distances is found by bisection on the value (0 .. 256: 9 steps), each
// step one ballot and one scalar popcount over the live lanes.  The running minimum of (median << 16 | i) is wave-uniform.
// No LDS, no atomics, no sort, integers only: equal inputs give equal bytes.
//
// Rows of 65 .. 256 entries run in the same kernel with four descriptors per lane (entry c * 64 + lane in chunk c).  That
// form was chosen over a workgroup per point because it keeps the one code path -- no LDS image of the descriptors, no
// barrier, no cross-wave minimum -- at 32 VGPRs of descriptors, which costs no occupancy that matters here; such rows are
// rare (the longest row of the measured world has 46 entries), and a list that has none never launches the second form.
//
// A point is a chain of three dependent gathers (slot -> row entries and record -> bad flags and descriptors).  The row
// does not wait for the record: entry e of a row lies inside the table whatever the count says.  A call lists a few
// thousand points, fewer waves than the device has wave slots, so every point's chain is in flight at once without a
// wave taking several points.
#include <hip/hip_runtime.h>

#include "obsgraph_kernels.h"

namespace orbfe {

namespace {

constexpr int kWave = 64;
constexpr int kDescThreads = 256, kDescWaves = kDescThreads / kWave;

template <int kChunks>
__global__ __launch_bounds__(kDescThreads) void k_obs_distinctive(ObsGraphDevice g, KfDescDevice kd, int n, const int32_t* __restrict__ slot,
                                                                  int32_t* __restrict__ bestKf, int32_t* __restrict__ bestIdx,
                                                                  uint8_t* __restrict__ outDesc, uint8_t* __restrict__ valid,
                                                                  MapPointsDevice table, int useTable) {
  const int i = __builtin_amdgcn_readfirstlane(blockIdx.x * kDescWaves + (int)threadIdx.x / kWave), lane = threadIdx.x % kWave;
  if (i >= n) return;  // (wave-uniform)
  const int s = slot[i];
  ObsEntry en[kChunks];
#pragma unroll
  for (int c = 0; c < kChunks; c++) {
    const int e = c * kWave + lane;
    en[c] = ObsEntry{0, 0, 0, 0};
    if (e < g.rowWidth) en[c] = g.rows[(size_t)s * g.rowWidth + e];
  }
  const ObsPointMeta m = g.meta[s];
  const bool dead = m.bad || m.count <= 0;  // mbBad: return (:278); observations.empty(): return (:283)
  // the short rows belong to the one-chunk form, which also answers for the points that have no row to read
  if (kChunks == 1 ? (!dead && m.count > kObsDescOneChunk) : (dead || m.count <= kObsDescOneChunk)) return;
  if (dead) {
    if (lane == 0) valid[i] = 0;
    return;
  }

  uint32_t d[kChunks][8];
  bool live[kChunks];
  unsigned long long mask[kChunks];
  int N = 0;
#pragma unroll
  for (int c = 0; c < kChunks; c++) {
    const bool in = c * kWave + lane < m.count;
    int bad = 1;
    uint4 a = make_uint4(0u, 0u, 0u, 0u), b = a;
    if (in) {  // the flag and the descriptor travel together; the host has checked idx against the key frame's count
      bad = g.kf[en[c].kf].bad;
      const uint4* p = reinterpret_cast<const uint4*>(kd.desc + ((size_t)en[c].kf * (size_t)kd.width + en[c].idx) * 32);
      a = p[0];
      b = p[1];
    }
    d[c][0] = a.x; d[c][1] = a.y; d[c][2] = a.z; d[c][3] = a.w;
    d[c][4] = b.x; d[c][5] = b.y; d[c][6] = b.z; d[c][7] = b.w;
    live[c] = in && !bad;  // !pKF->isBad() (:292)
    mask[c] = __ballot(live[c]);
    N += __popcll(mask[c]);
  }
  if (N == 0) {  // vDescriptors.empty(): return (:296)
    if (lane == 0) valid[i] = 0;
    return;
  }
  const int k = (N - 1) / 2;  // (size_t)(0.5 * (N - 1)) for N >= 1 (:321)

  unsigned best = 0xffffffffu;  // median << 16 | row position: the least key is the first row with the least median (:323)
#pragma unroll
  for (int c = 0; c < kChunks; c++) {
    unsigned long long todo = mask[c];
    while (todo) {  // (wave-uniform) the live entries of the chunk in row order
      const int l = __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      uint32_t r[8];
#pragma unroll
      for (int w = 0; w < 8; w++) r[w] = (uint32_t)__builtin_amdgcn_readlane((int)d[c][w], l);
      int dist[kChunks];
#pragma unroll
      for (int c2 = 0; c2 < kChunks; c2++) {
        int sum = 0;
#pragma unroll
        for (int w = 0; w < 8; w++) sum += __popc(r[w] ^ d[c2][w]);
        dist[c2] = sum;
      }
      // the least v with more than k distances <= v: vDists[k] after the sort (:320-321)
      int lo = 0, hi = 256;
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        int below = 0;
#pragma unroll
        for (int c2 = 0; c2 < kChunks; c2++) below += __popcll(__ballot(live[c2] && dist[c2] <= mid));
        if (below > k) hi = mid;
        else lo = mid + 1;
      }
      const unsigned key = ((unsigned)lo << 16) | (unsigned)(c * kWave + l);
      best = key < best ? key : best;
    }
  }

  // the winner's lane writes what it holds: mDescriptor = vDescriptors[BestIdx].clone() (:332)
  const int w = (int)(best & 0xffffu);
  uint4* out = reinterpret_cast<uint4*>(useTable ? table.desc + (size_t)s * 32 : outDesc + (size_t)i * 32);
#pragma unroll
  for (int c = 0; c < kChunks; c++) {
    if (w == c * kWave + lane) {
      out[0] = make_uint4(d[c][0], d[c][1], d[c][2], d[c][3]);
      out[1] = make_uint4(d[c][4], d[c][5], d[c][6], d[c][7]);
      bestKf[i] = en[c].kf;
      bestIdx[i] = en[c].idx;
      valid[i] = 1;
    }
  }
}

}  // namespace

void launch_obs_distinctive(hipStream_t s, const ObsGraphDevice& g, const KfDescDevice& kd, int n, const int32_t* slot, int maxCount,
                            int32_t* bestKf, int32_t* bestIdx, uint8_t* outDesc, uint8_t* valid, const MapPointsDevice* table) {
  if (n <= 0) return;
  const dim3 grid((unsigned)((n + kDescWaves - 1) / kDescWaves)), block(kDescThreads);
  const MapPointsDevice t = table ? *table : MapPointsDevice{};
  hipLaunchKernelGGL(k_obs_distinctive<1>, grid, block, 0, s, g, kd, n, slot, bestKf, bestIdx, outDesc, valid, t, table ? 1 : 0);
  if (maxCount > kObsDescOneChunk)
    hipLaunchKernelGGL(k_obs_distinctive<4>, grid, block, 0, s, g, kd, n, slot, bestKf, bestIdx, outDesc, valid, t, table ? 1 : 0);
}

}  // namespace orbfe
