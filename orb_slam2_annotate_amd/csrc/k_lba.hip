// k_lba.hip -- the passes of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:483-814) and BundleAdjustment (:54-253).
// The arithmetic and the work items are lba_math.h (binary64; the build has -ffp-contract=off); this file maps them onto
// threads and waves.  The host (lba.hip, lba_host.h) drives g2o's Levenberg loop and reads one LbaRecord per pass.
//
// Summation orders, functions of the problem's shape only (the CPU program of tests/cpp/lba_cpu.cpp repeats them):
//   Hll, b_l, a point's robust chi2     one thread per point, its edges ascending
//   Hpp, b_p of a free pose             64 lanes, lane l takes entries l, l + 64, ... of the pose's edge list (ascending edge
//                                       id), then __shfl_down with offsets 32, 16, 8, 4, 2, 1; lane 0 holds the total
//   a block of Hschur, bschur           the same lanes and tree over the edge list of the block's first pose
//   the Cholesky factor, substitutions  every element has one owner per elimination step: no sum is split
//   x_l of a point                      one thread per point, its edges ascending, the six terms of an edge in order
//   robust chi2, computeScale, maxima   one wave: lane l adds free poses l, l + 64, ... then points l, l + 64, ...; the tree
// Nothing else adds floating-point numbers; there is no atomic on one.
#include <hip/hip_runtime.h>

#include "lba_kernels.h"

namespace orbfe {
namespace {

__device__ __forceinline__ double wave_sum0(double v) {  // lane 0 holds the total
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
  return v;
}
__device__ __forceinline__ double wave_max0(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = fmax(v, __shfl_down(v, off));
  return v;
}
__device__ __forceinline__ int wave_count0(int v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
  return v;
}

__global__ __launch_bounds__(kLbaThreads) void k_lba_linearise(LbaArgs a, int cur, int robust) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p < a.nPoints) lba_linearise_point(a, p, cur, robust != 0);
}

__global__ __launch_bounds__(kLbaLanes) void k_lba_pose_blocks(LbaArgs a) {
  const int f = blockIdx.x, lane = threadIdx.x;
  double acc[kLbaPoseSums];
  int n;
  lba_pose_block_lane(a, f, lane, acc, &n);
#pragma unroll
  for (int k = 0; k < kLbaPoseSums; k++) acc[k] = wave_sum0(acc[k]);
  n = wave_count0(n);
  if (lane == 0) lba_pose_block_finish(a, f, acc, n);
}

__global__ __launch_bounds__(kLbaLanes) void k_lba_record(LbaArgs a, int ok) {
  LbaTotals t;
  lba_totals_lane(a, threadIdx.x, &t);
  t.chi2 = wave_sum0(t.chi2);
  t.scale = wave_sum0(t.scale);
  t.maxDiag = wave_max0(t.maxDiag);
  t.nActive = wave_count0(t.nActive);
  if (threadIdx.x == 0) {
    a.rec->chi2 = t.chi2; a.rec->scale = t.scale; a.rec->maxDiag = t.maxDiag; a.rec->nActive = t.nActive;
    if (ok) a.rec->ok = 1;  // (after a trial the solve has written it)
  }
}

__global__ __launch_bounds__(kLbaThreads) void k_lba_schur_points(LbaArgs a, double lambda) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p < a.nPoints) lba_schur_point(a, p, lambda);
}

// blocks [0, nBlocks): an upper block of Hschur; [nBlocks, nBlocks + nFree): a pose's bschur
__global__ __launch_bounds__(kLbaLanes) void k_lba_schur_blocks(LbaArgs a, int nBlocks, double lambda) {
  const int b = blockIdx.x, lane = threadIdx.x;
  if (b < nBlocks) {
    const int i1 = a.blockPose[2 * b], i2 = a.blockPose[2 * b + 1];
    double acc[kLbaBlockSums];
    lba_schur_block_lane(a, i1, i2, lane, acc);
#pragma unroll
    for (int k = 0; k < kLbaBlockSums; k++) acc[k] = wave_sum0(acc[k]);
    if (lane == 0) lba_schur_block_finish(a, i1, i2, acc, lambda);
  } else {
    const int f = b - nBlocks;
    double acc[6];
    lba_schur_rhs_lane(a, f, lane, acc);
#pragma unroll
    for (int k = 0; k < 6; k++) acc[k] = wave_sum0(acc[k]);
    if (lane == 0) lba_schur_rhs_finish(a, f, acc);
  }
}

// One workgroup: Cholesky of S (global memory, n = 6 nFree), the two substitutions, then the trial of every pose.  A
// non-positive pivot ends the factorisation: ok = 0 and a zero step, as a failed solve of section 4.L.  The flag lives in
// LDS and every thread reads it behind a barrier, so the exit is uniform.
__global__ __launch_bounds__(kLbaSolveThreads) void k_lba_solve(LbaArgs a, int cur, double lambda) {
  __shared__ int okS;
  __shared__ double colS[6 * kLbaSolveMaxPoses];
  const int tid = threadIdx.x;
  const size_t n = 6 * (size_t)a.nFree;
  double* S = a.S;
  if (tid == 0) okS = 1;
  __syncthreads();
  for (size_t j = 0; j < n; j++) {
    if (tid == 0 && !lba_chol_pivot(S, n, j)) okS = 0;
    __syncthreads();
    if (!okS) break;
    // scale column j and keep it in LDS: every update of the trailing triangle reads two of its entries
    for (size_t i = j + 1 + tid; i < n; i += kLbaSolveThreads) {
      lba_chol_scale(S, n, j, i);
      colS[i] = S[i * n + j];
    }
    __syncthreads();
    // the trailing lower triangle (i, k), j < k <= i: a wave takes rows i, i + 4, ..., its lanes consecutive k of the row
    // (lba_chol_update's arithmetic on the LDS copy of column j, which is not written here)
    for (size_t i = j + 1 + (tid >> 6); i < n; i += kLbaSolveThreads / 64) {
      const double lij = colS[i];
      for (size_t k = j + 1 + (tid & 63); k <= i; k += 64) S[i * n + k] = S[i * n + k] - lij * colS[k];
    }
    __syncthreads();
  }
  const bool ok = okS != 0;
  if (ok) {
    double* y = a.bs;
    for (size_t j = 0; j < n; j++) {  // L y = bschur, a column at a time
      if (tid == 0) y[j] = y[j] / S[j * n + j];
      __syncthreads();
      for (size_t i = j + 1 + tid; i < n; i += kLbaSolveThreads) y[i] = y[i] - S[i * n + j] * y[j];
      __syncthreads();
    }
    for (size_t jj = n; jj > 0; jj--) {  // L^T x = y
      const size_t j = jj - 1;
      if (tid == 0) y[j] = y[j] / S[j * n + j];
      __syncthreads();
      for (size_t i = tid; i < j; i += kLbaSolveThreads) y[i] = y[i] - S[j * n + i] * y[j];
      __syncthreads();
    }
    for (size_t i = tid; i < n; i += kLbaSolveThreads) a.xp[i] = y[i];
  } else {
    for (size_t i = tid; i < n; i += kLbaSolveThreads) a.xp[i] = 0.0;
  }
  if (tid == 0) a.rec->ok = ok ? 1 : 0;
  __syncthreads();
  for (int j = tid; j < a.nPoses; j += kLbaSolveThreads) lba_pose_trial(a, j, cur, lambda);
}

__global__ __launch_bounds__(kLbaThreads) void k_lba_trial_points(LbaArgs a, int cur, double lambda, int robust) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p < a.nPoints) lba_trial_point(a, p, cur, lambda, robust != 0, a.rec->ok != 0);
}

__global__ __launch_bounds__(kLbaThreads) void k_lba_classify(LbaArgs a, int cur, int final, uint8_t* erase) {
  const int e = blockIdx.x * kLbaThreads + threadIdx.x;
  if (e >= a.nEdges) return;
  const bool bad = lba_edge_bad(a, e, cur);
  if (final) erase[e] = bad ? (a.level[e] != 0 ? 1 : 2) : 0;
  else if (bad) a.level[e] = 1;
}

__global__ __launch_bounds__(kLbaThreads) void k_lba_gather(LbaArgs a, MapPointsDevice t, const int32_t* slot) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p >= a.nPoints) return;
  const float4 r = t.rec[2 * (size_t)slot[p]];
  double* X = lba_pt_at(a, 0, p);
  X[0] = (double)r.x; X[1] = (double)r.y; X[2] = (double)r.z;
}
__global__ __launch_bounds__(kLbaThreads) void k_lba_scatter(LbaArgs a, int cur, MapPointsDevice t, const int32_t* slot) {
  const int p = blockIdx.x * kLbaThreads + threadIdx.x;
  if (p >= a.nPoints) return;
  const double* X = lba_pt_at(a, cur, p);
  float4* r = t.rec + 2 * (size_t)slot[p];  // SetWorldPos(Converter::toCvMat(vPoint->estimate())): double -> float
  r->x = (float)X[0]; r->y = (float)X[1]; r->z = (float)X[2];
}

inline int blocks_of(int n) { return (n + kLbaThreads - 1) / kLbaThreads; }

}  // namespace

void launch_lba_linearise(hipStream_t s, const LbaArgs& a, int cur, int robust) {
  hipLaunchKernelGGL(k_lba_linearise, dim3(blocks_of(a.nPoints)), dim3(kLbaThreads), 0, s, a, cur, robust);
  if (a.nFree > 0) hipLaunchKernelGGL(k_lba_pose_blocks, dim3(a.nFree), dim3(kLbaLanes), 0, s, a);
  hipLaunchKernelGGL(k_lba_record, dim3(1), dim3(kLbaLanes), 0, s, a, 1);
}

void launch_lba_trial(hipStream_t s, const LbaArgs& a, int cur, double lambda, int robust) {
  hipLaunchKernelGGL(k_lba_schur_points, dim3(blocks_of(a.nPoints)), dim3(kLbaThreads), 0, s, a, lambda);
  const int nBlocks = a.nFree * (a.nFree + 1) / 2;
  if (a.nFree > 0) hipLaunchKernelGGL(k_lba_schur_blocks, dim3(nBlocks + a.nFree), dim3(kLbaLanes), 0, s, a, nBlocks, lambda);
  hipLaunchKernelGGL(k_lba_solve, dim3(1), dim3(kLbaSolveThreads), 0, s, a, cur, lambda);
  hipLaunchKernelGGL(k_lba_trial_points, dim3(blocks_of(a.nPoints)), dim3(kLbaThreads), 0, s, a, cur, lambda, robust);
  hipLaunchKernelGGL(k_lba_record, dim3(1), dim3(kLbaLanes), 0, s, a, 0);
}

void launch_lba_classify(hipStream_t s, const LbaArgs& a, int cur, int final, uint8_t* erase) {
  hipLaunchKernelGGL(k_lba_classify, dim3(blocks_of(a.nEdges)), dim3(kLbaThreads), 0, s, a, cur, final, erase);
}

void launch_lba_gather(hipStream_t s, const LbaArgs& a, const MapPointsDevice& t, const int32_t* slot) {
  hipLaunchKernelGGL(k_lba_gather, dim3(blocks_of(a.nPoints)), dim3(kLbaThreads), 0, s, a, t, slot);
}
void launch_lba_scatter(hipStream_t s, const LbaArgs& a, int cur, const MapPointsDevice& t, const int32_t* slot) {
  hipLaunchKernelGGL(k_lba_scatter, dim3(blocks_of(a.nPoints)), dim3(kLbaThreads), 0, s, a, cur, t, slot);
}

}  // namespace orbfe
