// k_stereopoints.hip -- the kernel of orbfe_create_stereo_points (include/orbfe.h; host side: stereopoints.hip; the
// arithmetic: stereopoints_host.h).  References: Tracking::CreateNewKeyFrame (src/Tracking.cc:1182-1234),
// Tracking::UpdateLastFrame (:899-949), Tracking::StereoInitialization (:563-578), Frame::UnprojectStereo
// (src/Frame.cc:713-727).
//
// One workgroup of 1024 threads does the whole call: a frame has at most 16384 keypoints, and the walk is a chain of
// small steps that would otherwise be one launch each.
//   compact   the keypoints with depth > 0, in index order, as keys bits(z) << 32 | i (mode ALL: i alone); a ballot per
//             wave, the waves' counts through LDS
//   sort      bitonic, in LDS, ascending: positive floats order as their bit patterns and the index breaks ties, which
//             is std::sort's order of pair<float, int>.  Mode ALL keeps the index order and sorts nothing
//   stop      the lowest j >= 100 with z_j > th_depth, an integer minimum; the walk handles j + 1 candidates
//   count     the walked candidates that make a point (ALL: each; else: not occupied), prefix sums as for compact
//   write     only when the count fits `capacity`: created point number w takes newSlot[w]; position, normal, range,
//             descriptor and flags go straight into the table rows, the index list and `cleared` into the outputs
// The places come from prefix sums over positions, never from arrival order: equal inputs give equal tables.
#include <hip/hip_runtime.h>

#include <climits>

#include "stereopoints_host.h"
#include "stereopoints_kernels.h"

namespace orbfe {

namespace {

constexpr int kWave = 64, kSpWaves = kSpThreads / kWave;

// the exclusive prefix of `flag` over the workgroup's threads, on top of *carry, which advances by the tile's total
__device__ inline int sp_scan_tile(bool flag, int32_t* waveSum, int* carry) {
  const int lane = threadIdx.x % kWave, wave = threadIdx.x / kWave;
  const unsigned long long mask = __ballot(flag);
  if (lane == 0) waveSum[wave] = __popcll(mask);
  __syncthreads();
  int before = 0, all = 0;
  for (int w = 0; w < kSpWaves; w++) {
    const int c = waveSum[w];
    before += w < wave ? c : 0;
    all += c;
  }
  const int pos = *carry + before + __popcll(mask & ((1ull << lane) - 1ull));
  *carry += all;
  __syncthreads();  // waveSum is rewritten by the next tile
  return pos;
}

template <int kKeys>
__global__ __launch_bounds__(kSpThreads) void k_stereo_points(MapPointsDevice t, StereoPointsArgs a) {
  __shared__ unsigned long long key[kKeys];
  __shared__ int32_t waveSum[kSpWaves];
  __shared__ int32_t stopAt;
  const int tid = threadIdx.x;
  const int sortN = a.sortN < kKeys ? a.sortN : kKeys;
  const bool all = a.mode == ORBFE_STEREO_ALL;
  if (tid == 0) stopAt = INT_MAX;

  // compact (and cleared[] starts at 0)
  int m = 0;
  for (int base = 0; base < a.n; base += kSpThreads) {
    const int i = base + tid;
    uint32_t zb = 0;
    if (i < a.n) {
      zb = __float_as_uint(a.depth[i]);
      a.cleared[i] = 0;
    }
    const bool cand = i < a.n && sp_candidate(zb);
    const int pos = sp_scan_tile(cand, waveSum, &m);
    if (cand && pos < sortN) key[pos] = ((unsigned long long)(all ? 0u : zb) << 32) | (unsigned)i;
  }
  m = m < sortN ? m : sortN;  // (the host sized sortN from the same depths: never cut)
  for (int j = m + tid; j < sortN; j += kSpThreads) key[j] = ~0ull;
  __syncthreads();

  if (!all) {
    for (int k = 2; k <= sortN; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int p = tid; p < (sortN >> 1); p += kSpThreads) {
          const int lo = ((p & ~(j - 1)) << 1) | (p & (j - 1)), hi = lo | j;
          const unsigned long long x = key[lo], y = key[hi];
          if ((x > y) == ((lo & k) == 0)) {
            key[lo] = y;
            key[hi] = x;
          }
        }
        __syncthreads();
      }
    // (:1231) after candidate j: z_j > th_depth && nPoints > 100, nPoints == j + 1
    for (int j = kStereoMinWalk + tid; j < m; j += kSpThreads)
      if (__uint_as_float((uint32_t)(key[j] >> 32)) > a.thDepth) atomicMin(&stopAt, j);
    __syncthreads();
  }
  const int walked = stopAt == INT_MAX ? m : stopAt + 1;

  int created = 0;
  for (int base = 0; base < walked; base += kSpThreads) {
    const int j = base + tid;
    const bool make = j < walked && (all || !a.occupied || !a.occupied[(uint32_t)key[j]]);
    (void)sp_scan_tile(make, waveSum, &created);
  }
  if (tid == 0) {
    a.header[0] = created;
    a.header[1] = walked;
  }
  if (created > a.capacity) return;  // (uniform) neither table is touched

  const float top = a.scale[a.nLevels - 1];
  int w0 = 0;
  for (int base = 0; base < walked; base += kSpThreads) {
    const int j = base + tid;
    const int i = j < walked ? (int)(uint32_t)key[j] : 0;
    const bool make = j < walked && (all || !a.occupied || !a.occupied[i]);
    const int w = sp_scan_tile(make, waveSum, &w0);
    if (!make) continue;
    const size_t s = (size_t)a.newSlot[w];
    float P[3], nrm[3], lo, hi;
    sp_unproject(a.pose, a.invfx, a.invfy, a.x[i], a.y[i], a.depth[i], P);
    sp_normal_range(P, a.centre, a.scale[a.octave[i]], top, nrm, &lo, &hi);
    t.rec[2 * s] = make_float4(P[0], P[1], P[2], lo);
    t.rec[2 * s + 1] = make_float4(nrm[0], nrm[1], nrm[2], hi);
    const uint4* src = reinterpret_cast<const uint4*>(a.desc + 32 * (size_t)i);  // row i of the frame: the one observation's
    uint4* dst = reinterpret_cast<uint4*>(t.desc + 32 * s);
    dst[0] = src[0];
    dst[1] = src[1];
    t.flags[s] = (uint8_t)a.flags;
    a.createdIdx[w] = i;
    // (:1207-1211).  Another thread stored the 0 during compaction: the __syncthreads() in between order the two stores
    // to global memory at workgroup scope, and only this workgroup writes the array
    if (a.mode == ORBFE_STEREO_KEYFRAME && a.stale && a.stale[i]) a.cleared[i] = 1;
  }
}

}  // namespace

void launch_stereo_points(hipStream_t s, const MapPointsDevice& table, const StereoPointsArgs& a) {
  if (a.sortN <= kSpSmallKeys)
    hipLaunchKernelGGL(k_stereo_points<kSpSmallKeys>, dim3(1), dim3(kSpThreads), 0, s, table, a);
  else
    hipLaunchKernelGGL(k_stereo_points<kSpMaxKeys>, dim3(1), dim3(kSpThreads), 0, s, table, a);
}

}  // namespace orbfe
