// k_loopcorrect.hip -- kernels of the loop correction on the resident map points (include/orbfe.h:
// orbfe_correct_loop_mappoints, orbfe_gba_update_mappoints; host side: loopcorrect.hip).  References:
// LoopClosing::CorrectLoop (src/LoopClosing.cc:558-600) with MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:360-404), and
// the map-point loop of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:818-852).
//
// The reference visits the key frames one after another and lets the first one that lists a point correct it.  "First" is
// a number here, as in k_kfpoints.hip: position p = k * width + idx, k the key frame's place in the caller's list.  The
// claimant of a point is the integer minimum of the positions that name it, which no arrival order can change, and the
// place of a claimed point in the output is the count of claims at lower positions (ballots and prefix sums, no cursor).
// Launches on one stream; the kernel boundaries order the plain stores, the atomics and the plain loads:
//   k_lc_rank     rank[kf slot] = k for the listed key frames (a kf slot named twice keeps its first place)
//   k_lc_mark     first[slot] = INT32_MAX for every live entry (only touched slots are written: nothing to clear)
//   k_lc_skip     first[slot] = -1 for the skip list: no position is below it, so the point is never claimed
//   k_lc_min      atomicMin(&first[slot], p)
//   k_lc_keep     keep = live && first[slot] == p; one 64-bit ballot per chunk, one count per block
//   k_lc_scan     one workgroup: block counts -> exclusive prefixes, *count          (the host reads *count here)
//   k_lc_emit     slotOut / refOut [prefix + popcount of the keep bits below] = slot / k
//   k_lc_correct  one lane per claimed point: P <- corrected[k]^-1 .map( noncorrected[k] .map(P) ) in binary64
//   k_lc_normal   one wave per claimed point: k_obs_normal_depth's chain with the centre of an observer chosen by rank
//   k_lc_ow       the listed key frames' Ow <- owCorrected
//   k_lc_release  rank[kf slot] = -1
// No floating-point atomics: equal inputs give equal bits.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "essgraph_math.h"
#include "loopcorrect_host.h"
#include "loopcorrect_kernels.h"

namespace orbfe {

namespace {

constexpr int kWave = 64;
constexpr int kLcThreads = kLcBlockEntries, kLcWaves = kLcThreads / kWave;
static_assert(kLcWaves == kLcChunksPerBlock, "a wave owns one chunk of the block");

__global__ __launch_bounds__(kLcThreads) void k_lc_rank(LoopCorrectArgs a) {
  const int k = blockIdx.x * kLcThreads + threadIdx.x;
  if (k < a.K && a.firstOf[k] == k) a.rank[a.kfSlot[k]] = k;
}

__global__ __launch_bounds__(kLcThreads) void k_lc_release(LoopCorrectArgs a) {
  const int k = blockIdx.x * kLcThreads + threadIdx.x;
  if (k < a.K) a.rank[a.kfSlot[k]] = -1;
}

// what a lane reads of its position: the place k in the list, the point slot (-1: nothing there), whether it is live
struct LcLane {
  int32_t p, slot;
  int k;
  bool live;
};

__device__ inline LcLane lc_read(const ObsGraphDevice& g, const KfPointsDevice& t, const LoopCorrectArgs& a, bool needLive) {
  LcLane L;
  const long long p = (long long)blockIdx.x * kLcThreads + threadIdx.x, span = (long long)a.K * t.width;  // span < 2^31: checked by the host
  L.p = (int32_t)(p < span ? p : 0);
  L.slot = -1; L.k = 0; L.live = false;
  if (p >= span) return L;
  L.k = (int)(p / t.width);
  const int idx = (int)(p % t.width), kf = a.kfSlot[L.k];
  if (a.firstOf[L.k] != L.k) return L;  // a kf slot named twice contributes nothing the second time
  if (idx < t.len[kf]) L.slot = t.rows[(size_t)kf * t.width + idx];
  if (needLive && L.slot >= 0) L.live = !g.meta[L.slot].bad;  // !pMPi, isBad() (:570-573); never set counts as bad
  return L;
}

__global__ __launch_bounds__(kLcThreads) void k_lc_mark(ObsGraphDevice g, KfPointsDevice t, LoopCorrectArgs a) {
  const LcLane L = lc_read(g, t, a, true);
  if (L.live) a.first[L.slot] = INT_MAX;
}

__global__ __launch_bounds__(kLcThreads) void k_lc_skip(LoopCorrectArgs a) {
  const int i = blockIdx.x * kLcThreads + threadIdx.x;
  if (i < a.nSkip) a.first[a.skip[i]] = -1;  // mnCorrectedByKF == mpCurrentKF->mnId (:574)
}

__global__ __launch_bounds__(kLcThreads) void k_lc_min(ObsGraphDevice g, KfPointsDevice t, LoopCorrectArgs a) {
  const LcLane L = lc_read(g, t, a, true);
  if (L.live) atomicMin(&a.first[L.slot], L.p);  // an integer minimum: the same in any order
}

__global__ __launch_bounds__(kLcThreads) void k_lc_keep(ObsGraphDevice g, KfPointsDevice t, LoopCorrectArgs a) {
  __shared__ int32_t waveTotal[kLcWaves];
  const LcLane L = lc_read(g, t, a, true);
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const int32_t f = L.live ? a.first[L.slot] : -2;  // positions are never negative; -1 is the skip list's
  const unsigned long long mask = __ballot(f == L.p);
  if (lane == 0) {
    a.keepMask[(size_t)blockIdx.x * kLcChunksPerBlock + wave] = mask;
    waveTotal[wave] = __popcll(mask);
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    int all = 0;
    for (int w = 0; w < kLcWaves; w++) all += waveTotal[w];
    a.blockCount[blockIdx.x] = all;
  }
}

// one workgroup: the blocks' counts become exclusive prefixes, the total becomes *count
__global__ __launch_bounds__(kLcThreads) void k_lc_scan(LoopCorrectArgs a) {
  __shared__ int32_t waveSum[kLcWaves];
  const int tid = threadIdx.x, wave = tid / kWave, lane = tid % kWave;
  int carry = 0;
  for (int base = 0; base < a.nBlocks; base += kLcThreads) {
    const int i = base + tid;
    const int v = i < a.nBlocks ? a.blockCount[i] : 0;
    int x = v;
    for (int d = 1; d < kWave; d <<= 1) {
      const int y = __shfl_up(x, d);
      if (lane >= d) x += y;
    }
    if (lane == kWave - 1) waveSum[wave] = x;
    __syncthreads();
    int before = 0, all = 0;
    for (int w = 0; w < kLcWaves; w++) {
      before += w < wave ? waveSum[w] : 0;
      all += waveSum[w];
    }
    if (i < a.nBlocks) a.blockCount[i] = carry + before + x - v;
    carry += all;
    __syncthreads();  // waveSum is rewritten by the next tile
  }
  if (tid == 0) a.count[0] = carry;
}

__global__ __launch_bounds__(kLcThreads) void k_lc_emit(ObsGraphDevice g, KfPointsDevice t, LoopCorrectArgs a, int count) {
  const int wave = threadIdx.x / kWave, lane = threadIdx.x % kWave;
  const unsigned long long* masks = a.keepMask + (size_t)blockIdx.x * kLcChunksPerBlock;
  int before = 0;
  for (int w = 0; w < wave; w++) before += __popcll(masks[w]);
  const unsigned long long mask = masks[wave];
  const LcLane L = lc_read(g, t, a, false);
  const int pos = a.blockCount[blockIdx.x] + before + __popcll(mask & ((1ull << lane) - 1ull));
  if (((mask >> lane) & 1ull) && pos < count) {
    a.slotOut[pos] = L.slot;
    a.refOut[pos] = L.k;  // mnCorrectedReference (:585) as a place in the list
  }
}

// (:578-583) on the table's record: compute in double, store as float (essgraph_math.h)
__global__ __launch_bounds__(kLcThreads) void k_lc_correct(MapPointsDevice t, LoopCorrectArgs a, int count) {
  const int i = blockIdx.x * kLcThreads + threadIdx.x;
  if (i >= count) return;
  const int k = a.refOut[i];
  float4* rec = t.rec + 2 * (size_t)a.slotOut[i];
  const float P[3] = {rec->x, rec->y, rec->z};
  float o[3];
  ess_correct_point(a.noncorrected + 8 * (size_t)k, a.corrected + 8 * (size_t)k, P, o);
  rec->x = o[0]; rec->y = o[1]; rec->z = o[2];
}

// k_obs_normal_depth (k_obsgraph.hip) for the claimed points, one wave per point, with one difference: the camera centre
// of an observer.  The reference calls UpdateNormalAndDepth inside its loop over the key frames and SetPose at the end of
// each (:586, :600): a key frame at a rank below the claimant's has its corrected pose by then, every other one (the
// claimant itself, later ranks, key frames outside the list) the pose the graph holds.
__global__ __launch_bounds__(kLcThreads) void k_lc_normal(ObsGraphDevice g, MapPointsDevice table, LoopCorrectArgs a, int count) {
  const int i = blockIdx.x * kLcWaves + (int)threadIdx.x / kWave, lane = threadIdx.x % kWave;
  if (i >= count) return;  // (wave-uniform)
  const int s = a.slotOut[i], claimant = a.refOut[i];
  const ObsPointMeta m = g.meta[s];
  bool ok = !m.bad && m.count > 0 && m.ref >= 0;  // observations.empty(): return (:375)
  float nx = 0.0f, ny = 0.0f, nz = 0.0f, dist = 0.0f;
  int refOctave = -1;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f);
  if (ok) {
    r0 = table.rec[2 * (size_t)s];
    const float X = r0.x, Y = r0.y, Z = r0.z;
    for (int e0 = 0; e0 < m.count; e0 += kWave) {
      const int e = e0 + lane;
      const bool live = e < m.count;
      float tx = 0.0f, ty = 0.0f, tz = 0.0f, len = 0.0f;
      int kf = -1, oct = 0;
      if (live) {
        const ObsEntry en = g.rows[(size_t)s * g.rowWidth + e];
        kf = en.kf; oct = en.octave;
        const int r = a.rank[kf];
        const float* ow = r >= 0 && r < claimant ? a.owCorrected + 3 * (size_t)r : g.kf[kf].ow;
        const float dx = __fsub_rn(X, ow[0]), dy = __fsub_rn(Y, ow[1]), dz = __fsub_rn(Z, ow[2]);  // mWorldPos - Owi
        const double ddx = (double)dx, ddy = (double)dy, ddz = (double)dz;
        const double nrm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(ddx, ddx), __dmul_rn(ddy, ddy)), __dmul_rn(ddz, ddz)));
        const float inv = (float)__ddiv_rn(1.0, nrm);  // Mat / double: the matrix times (float)(1 / s)
        tx = __fmul_rn(dx, inv); ty = __fmul_rn(dy, inv); tz = __fmul_rn(dz, inv);
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
    ok = refOctave >= 0 && refOctave < a.nLevels;  // the reference key frame is in the row
  }
  if (lane != 0) return;
  a.validOut[i] = ok;
  if (!ok) return;
  const float inv = (float)__ddiv_rn(1.0, (double)m.count);  // normal / n (:402)
  nx = __fmul_rn(nx, inv); ny = __fmul_rn(ny, inv); nz = __fmul_rn(nz, inv);
  const float hi = __fmul_rn(dist, a.scale[refOctave]);      // mfMaxDistance (:400)
  const float lo = __fdiv_rn(hi, a.scale[a.nLevels - 1]);    // mfMinDistance (:401)
  r0.w = lo;
  table.rec[2 * (size_t)s] = r0;
  table.rec[2 * (size_t)s + 1] = make_float4(nx, ny, nz, hi);
}

__global__ __launch_bounds__(kLcThreads) void k_lc_ow(ObsGraphDevice g, LoopCorrectArgs a) {
  const int k = blockIdx.x * kLcThreads + threadIdx.x;
  if (k >= a.K || a.firstOf[k] != k) return;
  float* ow = g.kf[a.kfSlot[k]].ow;
  ow[0] = a.owCorrected[3 * (size_t)k]; ow[1] = a.owCorrected[3 * (size_t)k + 1]; ow[2] = a.owCorrected[3 * (size_t)k + 2];
}

// ---- the map-point loop of RunGlobalBundleAdjustment ----

__global__ __launch_bounds__(kLcThreads) void k_gba_index(GbaUpdateArgs a, int set) {
  const int j = blockIdx.x * kLcThreads + threadIdx.x;
  if (j < a.m) a.index[a.kfSlot[j]] = set ? j : -1;
}

__global__ __launch_bounds__(kLcThreads) void k_gba_update(ObsGraphDevice g, MapPointsDevice t, GbaUpdateArgs a) {
  const int i = blockIdx.x * kLcThreads + threadIdx.x;
  if (i >= a.n) return;
  const int s = a.slot[i];
  const ObsPointMeta m = g.meta[s];
  uint8_t moved = 0;
  if (!m.bad) {  // (:824)
    float4* rec = t.rec + 2 * (size_t)s;
    if (a.inGba[i]) {  // SetWorldPos(mPosGBA) (:830)
      rec->x = a.posGba[3 * (size_t)i]; rec->y = a.posGba[3 * (size_t)i + 1]; rec->z = a.posGba[3 * (size_t)i + 2];
      moved = 1;
    } else {
      const int j = m.ref >= 0 ? a.index[m.ref] : -1;
      if (j >= 0 && a.reached[j]) {  // pRefKF->mnBAGlobalForKF == nLoopKF (:837)
        const float P[3] = {rec->x, rec->y, rec->z};
        float o[3];
        lc_gba_move(a.TcwBef + 16 * (size_t)j, a.TwcNew + 16 * (size_t)j, P, o);  // (:841-850)
        rec->x = o[0]; rec->y = o[1]; rec->z = o[2];
        moved = 2;
      }
    }
  }
  a.moved[i] = moved;
}

inline unsigned blocks_of(size_t n) { return (unsigned)((n + kLcThreads - 1) / kLcThreads); }

}  // namespace

void launch_lc_claim(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, const LoopCorrectArgs& a) {
  hipLaunchKernelGGL(k_lc_rank, dim3(blocks_of((size_t)a.K)), dim3(kLcThreads), 0, s, a);
  hipLaunchKernelGGL(k_lc_mark, dim3(a.nBlocks), dim3(kLcThreads), 0, s, g, t, a);
  if (a.nSkip > 0) hipLaunchKernelGGL(k_lc_skip, dim3(blocks_of((size_t)a.nSkip)), dim3(kLcThreads), 0, s, a);
  hipLaunchKernelGGL(k_lc_min, dim3(a.nBlocks), dim3(kLcThreads), 0, s, g, t, a);
  hipLaunchKernelGGL(k_lc_keep, dim3(a.nBlocks), dim3(kLcThreads), 0, s, g, t, a);
  hipLaunchKernelGGL(k_lc_scan, dim3(1), dim3(kLcThreads), 0, s, a);
}

void launch_lc_apply(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, const MapPointsDevice& table, const LoopCorrectArgs& a,
                     int count) {
  if (count > 0) {
    hipLaunchKernelGGL(k_lc_emit, dim3(a.nBlocks), dim3(kLcThreads), 0, s, g, t, a, count);
    hipLaunchKernelGGL(k_lc_correct, dim3(blocks_of((size_t)count)), dim3(kLcThreads), 0, s, table, a, count);
    hipLaunchKernelGGL(k_lc_normal, dim3((count + kLcWaves - 1) / kLcWaves), dim3(kLcThreads), 0, s, g, table, a, count);
  }
  hipLaunchKernelGGL(k_lc_ow, dim3(blocks_of((size_t)a.K)), dim3(kLcThreads), 0, s, g, a);
}

void launch_lc_release(hipStream_t s, const LoopCorrectArgs& a) {
  hipLaunchKernelGGL(k_lc_release, dim3(blocks_of((size_t)a.K)), dim3(kLcThreads), 0, s, a);
}

void launch_gba_update(hipStream_t s, const ObsGraphDevice& g, const MapPointsDevice& table, const GbaUpdateArgs& a) {
  if (a.m > 0) hipLaunchKernelGGL(k_gba_index, dim3(blocks_of((size_t)a.m)), dim3(kLcThreads), 0, s, a, 1);
  hipLaunchKernelGGL(k_gba_update, dim3(blocks_of((size_t)a.n)), dim3(kLcThreads), 0, s, g, table, a);
  if (a.m > 0) hipLaunchKernelGGL(k_gba_index, dim3(blocks_of((size_t)a.m)), dim3(kLcThreads), 0, s, a, 0);
}

}  // namespace orbfe
