// k_kfpoints.hip -- kernels over KeyFrame::mvpMapPoints, the rows of point slots per kf slot of the device observation
// graph (include/orbfe.h: orbfe_obsgraph_keyframe_points_union / _tracked_points; host side: kfpoints.hip).
// References: Tracking::UpdateLocalPoints (src/Tracking.cc:1315-1333), LocalMapping::SearchInNeighbors
// (src/LocalMapping.cc:555-571), LoopClosing::ComputeSim3 (src/LoopClosing.cc:420-436) -> the ordered union;
// KeyFrame::TrackedMapPoints (src/KeyFrame.cc:264-289) -> k_kf_tracked.
//
// The union keeps the FIRST occurrence of every live point in visiting order.  Visiting order is a number: position
// p = k * width + idx, k the key frame's place in the query.  So "first" is an integer minimum per point slot, which no
// arrival order can change, and the output place of a kept entry is the count of kept entries at lower positions, which
// ballots and prefix sums give without a cursor.  Five launches on one stream; the kernel boundaries are what order the
// plain stores, the atomics and the plain loads of consecutive passes (no flag, no spin, no cooperative launch):
//   k_kf_mark   first[q][slot] = INT32_MAX for every live entry (only touched slots are written: nothing to clear, and
//               racing stores write one value)
//   k_kf_min    atomicMin(&first[q][slot], p)
//   k_kf_keep   keep = live && first[q][slot] == p; one 64-bit ballot per chunk, one count per block
//   k_kf_scan   one workgroup per query: block counts -> exclusive prefixes, count[q]
//   k_kf_emit   out[q][prefix + popcount of the keep bits below] = slot
// All five are gathers with dependent latency (row entry -> point record -> first[]): a wave owns four consecutive
// chunks of a 1024-position block and issues the four loads of each stage together.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "obsgraph_kernels.h"

namespace orbfe {

namespace {

constexpr int kWave = 64;
constexpr int kKfThreads = 256, kKfWaves = kKfThreads / kWave, kKfUnroll = kKfChunksPerBlock / kKfWaves;
static_assert(kKfWaves * kKfUnroll * kWave == kKfBlockEntries, "a wave owns kKfUnroll chunks of the block");

__global__ __launch_bounds__(kKfThreads) void k_kf_scatter(KfPointsDevice t, int n, const int32_t* __restrict__ kf,
                                                           const int32_t* __restrict__ len, const int32_t* __restrict__ rowOf,
                                                           const int32_t* __restrict__ rows) {
  const size_t total = (size_t)n * t.width;
  for (size_t i = (size_t)blockIdx.x * kKfThreads + threadIdx.x; i < total; i += (size_t)gridDim.x * kKfThreads) {
    const int r = (int)(i / t.width), e = (int)(i % t.width);
    const int k = kf[r], src = rowOf[r];
    if (src >= 0 && e < len[r]) t.rows[(size_t)k * t.width + e] = rows[(size_t)src * t.width + e];
    if (e == 0) t.len[k] = len[r];
  }
}

// the query of a block of the flat grid: the last q with blkOff[q] <= blk (queries without blocks are passed over)
__device__ inline int query_of_block(const int32_t* __restrict__ blkOff, int nQueries, int blk) {
  int lo = 0, hi = nQueries;  // blkOff[lo] <= blk < blkOff[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (blkOff[mid] <= blk) lo = mid;
    else hi = mid;
  }
  return lo;
}

// What a wave reads of its kKfUnroll chunks: per lane the position, the point slot (-1: nothing there) and whether the
// point is live.  The loads of one stage are issued together.
struct KfLane {
  int q;
  int32_t p[kKfUnroll], slot[kKfUnroll];
  bool live[kKfUnroll];
};

__device__ inline void kf_read(const ObsGraphDevice& g, const KfPointsDevice& t, const KfUnionArgs& a, bool needLive, KfLane* L) {
  const int blk = blockIdx.x, wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int q = query_of_block(a.blkOff, a.nQueries, blk);
  const int k0 = a.qOff[q], nKf = a.qOff[q + 1] - k0;
  const int32_t span = nKf * t.width;  // < 2^31: checked by the host
  const int32_t base = (blk - a.blkOff[q]) * kKfBlockEntries + wave * kKfUnroll * kWave;
  L->q = q;
  int kf[kKfUnroll], idx[kKfUnroll], len[kKfUnroll];
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) {
    const int32_t p0 = base + u * kWave;  // the chunk lies in one row: width is a multiple of 64
    L->p[u] = p0 + lane;
    kf[u] = -1;
    idx[u] = p0 % t.width + lane;
    if (p0 < span) kf[u] = a.qKf[k0 + p0 / t.width];
  }
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) len[u] = kf[u] >= 0 ? t.len[kf[u]] : 0;
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) L->slot[u] = idx[u] < len[u] ? t.rows[(size_t)kf[u] * t.width + idx[u]] : -1;
  if (!needLive) return;
  int32_t bad[kKfUnroll];
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) bad[u] = L->slot[u] >= 0 ? g.meta[L->slot[u]].bad : 1;  // !pMP, isBad()
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) L->live[u] = !bad[u];
}

__global__ __launch_bounds__(kKfThreads) void k_kf_mark(ObsGraphDevice g, KfPointsDevice t, KfUnionArgs a) {
  KfLane L;
  kf_read(g, t, a, true, &L);
  int32_t* first = a.first + (size_t)L.q * g.pointCap;
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++)
    if (L.live[u]) first[L.slot[u]] = INT_MAX;
}

__global__ __launch_bounds__(kKfThreads) void k_kf_min(ObsGraphDevice g, KfPointsDevice t, KfUnionArgs a) {
  KfLane L;
  kf_read(g, t, a, true, &L);
  int32_t* first = a.first + (size_t)L.q * g.pointCap;
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++)
    if (L.live[u]) atomicMin(&first[L.slot[u]], L.p[u]);  // an integer minimum: the same in any order
}

__global__ __launch_bounds__(kKfThreads) void k_kf_keep(ObsGraphDevice g, KfPointsDevice t, KfUnionArgs a) {
  __shared__ int32_t waveTotal[kKfWaves];
  KfLane L;
  kf_read(g, t, a, true, &L);
  const int32_t* first = a.first + (size_t)L.q * g.pointCap;
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  int32_t f[kKfUnroll];
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) f[u] = L.live[u] ? first[L.slot[u]] : -1;  // positions are never negative
  int total = 0;
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) {
    const unsigned long long mask = __ballot(f[u] == L.p[u]);
    if (lane == 0) a.keepMask[(size_t)blockIdx.x * kKfChunksPerBlock + wave * kKfUnroll + u] = mask;
    total += __popcll(mask);
  }
  if (lane == 0) waveTotal[wave] = total;
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 0;
    for (int w = 0; w < kKfWaves; w++) all += waveTotal[w];
    a.blockCount[blockIdx.x] = all;
  }
}

// one workgroup per query: its blocks' counts become exclusive prefixes, the total becomes count[q]
__global__ __launch_bounds__(kKfThreads) void k_kf_scan(KfUnionArgs a) {
  __shared__ int32_t waveSum[kKfWaves];
  const int q = blockIdx.x, tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  const int lo = a.blkOff[q], hi = a.blkOff[q + 1];
  int carry = 0;
  for (int base = lo; base < hi; base += kKfThreads) {
    const int i = base + tid;
    const int v = i < hi ? a.blockCount[i] : 0;
    int x = v;
    for (int d = 1; d < kWave; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == kWave - 1) waveSum[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kKfWaves; w++) {
      before += w < wave ? waveSum[w] : 0;
      all += waveSum[w];
    }
    if (i < hi) a.blockCount[i] = carry + before + x - v;
    carry += all;
    __syncthreads();  // waveSum is rewritten by the next tile
  }
  if (tid == 0) a.count[q] = carry;
}

__global__ __launch_bounds__(kKfThreads) void k_kf_emit(ObsGraphDevice g, KfPointsDevice t, KfUnionArgs a) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  // the block's 16 keep masks, one per lane 0..15, and from them every chunk's place within the block
  const unsigned long long mine = lane < kKfChunksPerBlock ? a.keepMask[(size_t)blockIdx.x * kKfChunksPerBlock + lane] : 0ull;
  const int n = __popcll(mine);
  int incl = n;
  for (int d = 1; d < kKfChunksPerBlock; d <<= 1) {
    const int y = __shfl_up(incl, d);
    if (lane >= d) incl += y;
  }
  const int32_t blockBase = a.blockCount[blockIdx.x];
  KfLane L;
  kf_read(g, t, a, false, &L);
  int32_t* out = a.out + (size_t)L.q * a.capacity;
#pragma unroll
  for (int u = 0; u < kKfUnroll; u++) {
    const int c = wave * kKfUnroll + u;
    const unsigned long long mask = __shfl(mine, c);
    const int before = __shfl(incl - n, c);
    const int pos = blockBase + before + __popcll(mask & ((1ull << lane) - 1ull));
    if (((mask >> lane) & 1ull) && pos < a.capacity) out[pos] = L.slot[u];
  }
}

// one wave per key frame (:270-286): four chunks of the row in flight
__global__ __launch_bounds__(kKfThreads) void k_kf_tracked(ObsGraphDevice g, KfPointsDevice t, int n, const int32_t* __restrict__ kf,
                                                           int minObs, int32_t* __restrict__ count) {
  const int i = blockIdx.x * kKfWaves + (int)threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (i >= n) return;  // (wave-uniform)
  const int k = kf[i], len = t.len[k];
  const int32_t* row = t.rows + (size_t)k * t.width;
  int total = 0;
  for (int e0 = 0; e0 < len; e0 += kKfUnroll * kWave) {
    int32_t s[kKfUnroll];
    bool ok[kKfUnroll];
#pragma unroll
    for (int u = 0; u < kKfUnroll; u++) {
      const int e = e0 + u * kWave + lane;
      s[u] = e < len ? row[e] : -1;
    }
#pragma unroll
    for (int u = 0; u < kKfUnroll; u++) {
      ok[u] = false;
      if (s[u] >= 0) {  // pMP
        const ObsPointMeta m = g.meta[s[u]];
        ok[u] = !m.bad && (minObs > 0 ? m.nObs >= minObs : true);  // !isBad(); bCheckObs: Observations() >= minObs
      }
    }
#pragma unroll
    for (int u = 0; u < kKfUnroll; u++) total += __popcll(__ballot(ok[u]));
  }
  if (lane == 0) count[i] = total;
}

}  // namespace

void launch_kf_scatter(hipStream_t s, const KfPointsDevice& t, int n, const int32_t* kf, const int32_t* len, const int32_t* rowOf,
                       const int32_t* rows) {
  if (n <= 0) return;
  const size_t total = (size_t)n * t.width;
  const unsigned blocks = (unsigned)std::min<size_t>((total + kKfThreads - 1) / kKfThreads, 65535);
  hipLaunchKernelGGL(k_kf_scatter, dim3(blocks), dim3(kKfThreads), 0, s, t, n, kf, len, rowOf, rows);
}

void launch_kf_union(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, const KfUnionArgs& a) {
  if (a.nQueries <= 0) return;
  if (a.nBlocks > 0) {
    hipLaunchKernelGGL(k_kf_mark, dim3(a.nBlocks), dim3(kKfThreads), 0, s, g, t, a);
    hipLaunchKernelGGL(k_kf_min, dim3(a.nBlocks), dim3(kKfThreads), 0, s, g, t, a);
    hipLaunchKernelGGL(k_kf_keep, dim3(a.nBlocks), dim3(kKfThreads), 0, s, g, t, a);
  }
  hipLaunchKernelGGL(k_kf_scan, dim3(a.nQueries), dim3(kKfThreads), 0, s, a);
  if (a.nBlocks > 0) hipLaunchKernelGGL(k_kf_emit, dim3(a.nBlocks), dim3(kKfThreads), 0, s, g, t, a);
}

void launch_kf_tracked(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, int n, const int32_t* kf, int minObs,
                       int32_t* count) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_kf_tracked, dim3((n + kKfWaves - 1) / kKfWaves), dim3(kKfThreads), 0, s, g, t, n, kf, minObs, count);
}

}  // namespace orbfe
