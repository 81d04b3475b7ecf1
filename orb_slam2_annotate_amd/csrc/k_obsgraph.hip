// k_obsgraph.hip -- kernels of the device observation graph (include/orbfe.h: orbfe_obsgraph; host side: obsgraph.hip).
// References: KeyFrame::UpdateConnections (src/KeyFrame.cc:326-344) and Tracking::UpdateLocalKeyFrames
// (src/Tracking.cc:1346-1362) -> k_obs_votes; LocalMapping::KeyFrameCulling (src/LocalMapping.cc:729-769) ->
// k_obs_culling; MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:360-404) -> k_obs_normal_depth.
//
// All three are gathers over rows of a few dozen 8-byte entries: latency-bound, not bandwidth-bound.  A wave takes a
// point and its lanes read the row as one coalesced segment (row_width * 8 bytes, at most 2 KB); what hides the latency
// is many waves and, in the votes kernel where one workgroup owns a whole query, four rows in flight per wave.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "obsgraph_kernels.h"

namespace orbfe {

namespace {

constexpr int kWave = 64;
constexpr int kVotesThreads = 1024, kVotesWaves = kVotesThreads / kWave, kVotesUnroll = 4;
constexpr int kObsThreads = 256, kObsWaves = kObsThreads / kWave;

__global__ __launch_bounds__(kObsThreads) void k_obs_scatter(ObsGraphDevice g, int n, const int32_t* __restrict__ slot,
                                                             const ObsPointMeta* __restrict__ meta,
                                                             const int32_t* __restrict__ rowOf, const ObsEntry* __restrict__ rows) {
  const size_t total = (size_t)n * g.rowWidth;
  for (size_t t = (size_t)blockIdx.x * kObsThreads + threadIdx.x; t < total; t += (size_t)gridDim.x * kObsThreads) {
    const int i = (int)(t / g.rowWidth), e = (int)(t % g.rowWidth);
    const int s = slot[i], r = rowOf[i];
    if (r >= 0 && e < meta[i].count) g.rows[(size_t)s * g.rowWidth + e] = rows[(size_t)r * g.rowWidth + e];
    if (e == 0) g.meta[s] = meta[i];
  }
}

// the counters of one query: LDS (plain loads see the workgroup's LDS atomics behind a barrier), or the query's workspace
// slice, read back past the L1 that the atomics do not go through
template <bool kLds>
__device__ inline int32_t counter_load(const int32_t* p) {
  if (kLds) return *p;
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <bool kLds>
__global__ __launch_bounds__(kVotesThreads) void k_obs_votes(ObsGraphDevice g, const int32_t* __restrict__ qOff,
                                                             const int32_t* __restrict__ qSlots, const int32_t* __restrict__ self,
                                                             int capacity, int32_t* __restrict__ outKf,
                                                             int32_t* __restrict__ outWeight, int32_t* __restrict__ count,
                                                             int32_t* counters) {
  extern __shared__ int32_t ldsCounters[];
  __shared__ int32_t waveTotal[kVotesWaves];
  const int q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  int32_t* cnt = kLds ? ldsCounters : counters + (size_t)q * g.kfCap;
  for (int k = tid; k < g.kfCap; k += kVotesThreads) {
    if (kLds) cnt[k] = 0;
    else __hip_atomic_store(&cnt[k], 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  __syncthreads();

  // the votes: every entry of every live point's row, except the query's own key frame.  Integer adds: exact in any order
  const int n = qOff[q + 1] - qOff[q], me = self[q];
  const int32_t* sl = qSlots + qOff[q];
  for (int p0 = wave * kVotesUnroll; p0 < n; p0 += kVotesWaves * kVotesUnroll) {
    int s[kVotesUnroll], c[kVotesUnroll], most = 0;
#pragma unroll
    for (int u = 0; u < kVotesUnroll; u++) s[u] = p0 + u < n ? sl[p0 + u] : -1;
#pragma unroll
    for (int u = 0; u < kVotesUnroll; u++) {
      c[u] = 0;
      if (s[u] >= 0) {
        const ObsPointMeta m = g.meta[s[u]];
        c[u] = m.bad ? 0 : m.count;
      }
      most = c[u] > most ? c[u] : most;
    }
    for (int e0 = 0; e0 < most; e0 += kWave) {
      const int e = e0 + lane;
      int kf[kVotesUnroll];
#pragma unroll
      for (int u = 0; u < kVotesUnroll; u++) kf[u] = e < c[u] ? g.rows[(size_t)s[u] * g.rowWidth + e].kf : -1;
#pragma unroll
      for (int u = 0; u < kVotesUnroll; u++)
        if (kf[u] >= 0 && kf[u] != me) atomicAdd(&cnt[kf[u]], 1);
    }
  }
  __syncthreads();

  // compaction to ascending kf slot, by ballot and prefix popcount: wave w owns one contiguous run of 64-slot chunks,
  // counts its non-zero counters, and writes them behind the totals of the waves before it.  No cursor: equal inputs
  // give equal arrays.
  const int chunks = (g.kfCap + kWave - 1) / kWave, perWave = (chunks + kVotesWaves - 1) / kVotesWaves;
  const int k0 = wave * perWave * kWave, k1 = min(g.kfCap, k0 + perWave * kWave);
  int total = 0;
  for (int kb = k0; kb < k1; kb += kWave) {
    const int k = kb + lane;
    const int32_t v = k < k1 ? counter_load<kLds>(&cnt[k]) : 0;
    total += __popcll(__ballot(v > 0));
  }
  if (lane == 0) waveTotal[wave] = total;
  __syncthreads();
  int base = 0, all = 0;
  for (int w = 0; w < kVotesWaves; w++) {
    base += w < wave ? waveTotal[w] : 0;
    all += waveTotal[w];
  }
  for (int kb = k0; kb < k1; kb += kWave) {
    const int k = kb + lane;
    const int32_t v = k < k1 ? counter_load<kLds>(&cnt[k]) : 0;
    const unsigned long long mask = __ballot(v > 0);
    const int pos = base + __popcll(mask & ((1ull << lane) - 1ull));
    if (v > 0 && pos < capacity) {
      outKf[(size_t)q * capacity + pos] = k;
      outWeight[(size_t)q * capacity + pos] = v;
    }
    base += __popcll(mask);
  }
  if (tid == 0) count[q] = all;
}

// one wave per listed feature (:731-766)
__global__ __launch_bounds__(kObsThreads) void k_obs_culling(ObsGraphDevice g, int nFeatures, const int32_t* __restrict__ cand,
                                                             const int32_t* __restrict__ kfSlot, const int32_t* __restrict__ slot,
                                                             const uint8_t* __restrict__ octave, int32_t* nMps, int32_t* nRedundant) {
  const int f = blockIdx.x * kObsWaves + (int)threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (f >= nFeatures) return;  // (wave-uniform)
  const int s = slot[f], c = cand[f], level = octave[f], me = kfSlot[c];
  const ObsPointMeta m = g.meta[s];
  if (m.bad) return;  // pMP->isBad() (:734)
  if (lane == 0) atomicAdd(&nMps[c], 1);
  if (m.nObs <= 3) return;  // pMP->Observations() > thObs (:743)
  int n = 0;
  for (int e0 = 0; e0 < m.count; e0 += kWave) {
    const int e = e0 + lane;
    bool ok = false;
    if (e < m.count) {
      const ObsEntry en = g.rows[(size_t)s * g.rowWidth + e];
      ok = en.kf != me && (int)en.octave <= level + 1;  // pKFi == pKF: continue; scaleLeveli <= scaleLevel + 1
    }
    n += __popcll(__ballot(ok));
  }
  if (n >= 3 && lane == 0) atomicAdd(&nRedundant[c], 1);
}

// one wave per point: the lanes compute the terms of their entries, one chain adds them in row order.  Written with the
// round-to-nearest intrinsics in the order include/orbfe.h states: no contraction, no reassociation.
__global__ __launch_bounds__(kObsThreads) void k_obs_normal_depth(ObsGraphDevice g, int n, const int32_t* __restrict__ slot,
                                                                  const float* __restrict__ pos, const float* __restrict__ scale,
                                                                  int nLevels, float* __restrict__ normal, float* __restrict__ minDist,
                                                                  float* __restrict__ maxDist, uint8_t* __restrict__ valid,
                                                                  MapPointsDevice table, int useTable) {
  const int i = blockIdx.x * kObsWaves + (int)threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (i >= n) return;  // (wave-uniform)
  const int s = slot[i];
  const ObsPointMeta m = g.meta[s];
  bool ok = !m.bad && m.count > 0 && m.ref >= 0;  // mbBad: return (:368); observations.empty(): return (:375)
  float nx = 0.0f, ny = 0.0f, nz = 0.0f, dist = 0.0f;
  int refOctave = -1;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    float X, Y, Z;
    if (useTable) {
      r0 = table.rec[2 * (size_t)s];
      X = r0.x; Y = r0.y; Z = r0.z;
    } else {
      X = pos[3 * (size_t)i]; Y = pos[3 * (size_t)i + 1]; Z = pos[3 * (size_t)i + 2];
    }
    for (int e0 = 0; e0 < m.count; e0 += kWave) {
      const int e = e0 + lane;
      const bool live = e < m.count;
      float tx = 0.0f, ty = 0.0f, tz = 0.0f, len = 0.0f;
      int kf = -1, oct = 0;
      if (live) {
        const ObsEntry en = g.rows[(size_t)s * g.rowWidth + e];
        kf = en.kf; oct = en.octave;
        const ObsKeyFrame k = g.kf[en.kf];
        const float dx = __fsub_rn(X, k.ow[0]), dy = __fsub_rn(Y, k.ow[1]), dz = __fsub_rn(Z, k.ow[2]);  // mWorldPos - Owi
        const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
        const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz)));
        const float a = (float)__ddiv_rn(1.0, nrm);  // Mat / double: the matrix times (float)(1 / s)
        tx = __fmul_rn(dx, a); ty = __fmul_rn(dy, a); tz = __fmul_rn(dz, a);
        len = (float)nrm;
      }
      const unsigned long long isRef = __ballot(live && kf == m.ref);
      if (isRef && refOctave < 0) {  // PC = Pos - pRefKF->GetCameraCenter() is that lane's d, dist its norm (:389-391)
        const int src = __ffsll((long long)isRef) - 1;
        refOctave = __shfl(oct, src);
        dist = __shfl(len, src);
      }
      const int here = min(kWave, m.count - e0);
      for (int j = 0; j < here; j++) {  // normal = normal + normali / norm, in row order (:385)
        nx = __fadd_rn(nx, __shfl(tx, j));
        ny = __fadd_rn(ny, __shfl(ty, j));
        nz = __fadd_rn(nz, __shfl(tz, j));
      }
    }
    ok = refOctave >= 0 && refOctave < nLevels;  // the reference key frame is in the row
  }
  if (lane != 0) return;
  valid[i] = ok;
  if (!ok) return;
  const float inv = (float)__ddiv_rn(1.0, (double)m.count);  // normal / n (:402)
  nx = __fmul_rn(nx, inv); ny = __fmul_rn(ny, inv); nz = __fmul_rn(nz, inv);
  const float hi = __fmul_rn(dist, scale[refOctave]);   // mfMaxDistance (:400)
  const float lo = __fdiv_rn(hi, scale[nLevels - 1]);   // mfMinDistance (:401)
  if (useTable) {
    r0.w = lo;
    table.rec[2 * (size_t)s] = r0;
    table.rec[2 * (size_t)s + 1] = make_float4(nx, ny, nz, hi);
  } else {
    normal[3 * (size_t)i] = nx; normal[3 * (size_t)i + 1] = ny; normal[3 * (size_t)i + 2] = nz;
    minDist[i] = lo;
    maxDist[i] = hi;
  }
}

}  // namespace

void launch_obs_scatter(hipStream_t s, const ObsGraphDevice& g, int n, const int32_t* slot, const ObsPointMeta* meta,
                        const int32_t* rowOf, const ObsEntry* rows) {
  if (n <= 0) return;
  const size_t total = (size_t)n * g.rowWidth;
  const unsigned blocks = (unsigned)std::min<size_t>((total + kObsThreads - 1) / kObsThreads, 65535);
  hipLaunchKernelGGL(k_obs_scatter, dim3(blocks), dim3(kObsThreads), 0, s, g, n, slot, meta, rowOf, rows);
}

void launch_obs_votes(hipStream_t s, const ObsGraphDevice& g, int nQueries, const int32_t* qOff, const int32_t* qSlots,
                      const int32_t* self, int capacity, int32_t* outKf, int32_t* outWeight, int32_t* count, int32_t* counters) {
  if (nQueries <= 0) return;
  if (g.kfCap <= kObsVotesLdsKeyFrames)
    hipLaunchKernelGGL(k_obs_votes<true>, dim3(nQueries), dim3(kVotesThreads), (size_t)g.kfCap * sizeof(int32_t), s, g, qOff, qSlots,
                       self, capacity, outKf, outWeight, count, counters);
  else
    hipLaunchKernelGGL(k_obs_votes<false>, dim3(nQueries), dim3(kVotesThreads), 0, s, g, qOff, qSlots, self, capacity, outKf,
                       outWeight, count, counters);
}

void launch_obs_culling(hipStream_t s, const ObsGraphDevice& g, int nFeatures, const int32_t* cand, const int32_t* kfSlot,
                        const int32_t* slot, const uint8_t* octave, int32_t* nMps, int32_t* nRedundant) {
  if (nFeatures <= 0) return;
  hipLaunchKernelGGL(k_obs_culling, dim3((nFeatures + kObsWaves - 1) / kObsWaves), dim3(kObsThreads), 0, s, g, nFeatures, cand, kfSlot,
                     slot, octave, nMps, nRedundant);
}

void launch_obs_normal_depth(hipStream_t s, const ObsGraphDevice& g, int n, const int32_t* slot, const float* pos,
                             const float* scale, int nLevels, float* normal, float* minDist, float* maxDist, uint8_t* valid,
                             const MapPointsDevice* table) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_obs_normal_depth, dim3((n + kObsWaves - 1) / kObsWaves), dim3(kObsThreads), 0, s, g, n, slot, pos, scale, nLevels,
                     normal, minDist, maxDist, valid, table ? *table : MapPointsDevice{}, table ? 1 : 0);
}

}  // namespace orbfe
