// k_essgraph.hip -- the kernels of Optimizer::OptimizeEssentialGraph (gfx950): the work items of essgraph_math.h, one per
// lane.  Summation orders:
//   an element of a block of H, of b      one lane, the block's edges ascending, the seven products of an edge in row order
//   an element of the factor              one owner per step, its updates in ascending column order
//   the substitutions                     one owner per component and step
//   chi2, computeScale's sum              64 lane-strided partial sums, then __shfl_down with offsets 32 .. 1; lane 0's total
// The factorisation is ONE workgroup that walks the block columns with workgroup barriers.  Every loop bound comes from the
// host-built tables (colptr), a failed pivot only raises a flag in LDS and the loops run on: no thread can skip a barrier.
#include <hip/hip_runtime.h>

#include "essgraph_kernels.h"

namespace orbfe {
namespace {

__device__ __forceinline__ double ess_wave_sum0(double v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v = v + __shfl_down(v, off);
  return v;
}

__global__ __launch_bounds__(kEssThreads) void k_ess_measure(EssArgs a) {
  const int e = blockIdx.x * kEssThreads + threadIdx.x;
  if (e < a.nEdges) ess_measure_edge(a, e);
}

__global__ __launch_bounds__(kEssThreads) void k_ess_linearise(EssArgs a, int cur) {
  const int k = blockIdx.x * kEssThreads + threadIdx.x;
  if (k < a.nActive) ess_linearise_item(a, k, cur);
}

__global__ __launch_bounds__(kEssLanes) void k_ess_assemble(EssArgs a) {
  const int t = blockIdx.x;
  if (t < a.blocksA) ess_assemble_lane(a, t, threadIdx.x);
}

__global__ __launch_bounds__(kEssLanes) void k_ess_record(EssArgs a, double lambda, int setOk) {
  double c, s;
  ess_record_lane(a, threadIdx.x, lambda, &c, &s);
  c = ess_wave_sum0(c);
  s = ess_wave_sum0(s);
  if (threadIdx.x == 0) {
    a.rec->chi2 = c;
    a.rec->scale = s;
    a.rec->maxDiag = 0.0;
    a.rec->nActive = a.nActive;
    if (setOk) a.rec->ok = 1;
  }
}

__global__ __launch_bounds__(kEssThreads) void k_ess_load(EssArgs a, double lambda) {
  const size_t i = (size_t)blockIdx.x * kEssThreads + threadIdx.x;
  if (i < 49 * (size_t)a.blocksL) ess_load_element(a, i, lambda);
}

__global__ __launch_bounds__(kEssFactorThreads) void k_ess_factor(EssArgs a, int cur, int doTrial) {
  __shared__ int failS;
  const int tid = threadIdx.x;
  const int n = a.nFree;
  double* L = a.L;
  double* x = a.x;
  if (tid == 0) failS = 0;
  __syncthreads();
  for (int j = 0; j < n; j++) {
    const int p0 = a.colptr[j], p1 = a.colptr[j + 1];
    const int nEl = 49 * (p1 - p0);
    for (int i = tid; i < nEl; i += kEssFactorThreads) ess_chol_update_element(a.updOff, a.updSrc, L, p0 + i / 49, i % 49);
    __syncthreads();
    if (tid == 0 && !ess_chol_diag(L + 49 * (size_t)p0)) failS = 1;
    __syncthreads();
    const int nRows = 7 * (p1 - p0 - 1);
    for (int i = tid; i < nRows; i += kEssFactorThreads) ess_chol_scale_row(L + 49 * (size_t)p0, L + 49 * (size_t)(p0 + 1 + i / 7), i % 7);
    __syncthreads();
  }
  for (int j = 0; j < n; j++) {  // L y = b
    const int p0 = a.colptr[j], p1 = a.colptr[j + 1];
    if (tid == 0) ess_fwd_diag(L + 49 * (size_t)p0, x + 7 * (size_t)j);
    __syncthreads();
    const int nRows = 7 * (p1 - p0 - 1);
    for (int i = tid; i < nRows; i += kEssFactorThreads) {
      const int p = p0 + 1 + i / 7;
      ess_fwd_row(L + 49 * (size_t)p, x + 7 * (size_t)j, x + 7 * (size_t)a.rowidx[p], i % 7);
    }
    __syncthreads();
  }
  for (int j = n - 1; j >= 0; j--) {  // L^T x = y
    if (tid < 7) ess_bwd_component(a.colptr, a.rowidx, L, x, j, tid);
    __syncthreads();
    if (tid == 0) ess_bwd_diag(L + 49 * (size_t)a.colptr[j], x + 7 * (size_t)j);
    __syncthreads();
  }
  const bool ok = failS == 0;
  if (!ok)  // a failed factorisation is a zero step
    for (int i = tid; i < 7 * n; i += kEssFactorThreads) x[i] = 0.0;
  if (tid == 0) a.rec->ok = ok ? 1 : 0;
  __syncthreads();
  if (doTrial)
    for (int f = tid; f < n; f += kEssFactorThreads) ess_trial_vertex(a, f, cur);
}

__global__ __launch_bounds__(kEssThreads) void k_ess_trial_edges(EssArgs a, int cur) {
  const int k = blockIdx.x * kEssThreads + threadIdx.x;
  if (k < a.nActive) ess_trial_edge(a, k, cur);
}

__global__ __launch_bounds__(kEssThreads) void k_ess_correct_points(const double* sim3, const double* sim3Out, int nPoints, const float* xw,
                                                                    const int32_t* refVertex, float* xwOut) {
  const int p = blockIdx.x * kEssThreads + threadIdx.x;
  if (p >= nPoints) return;
  const float P[3] = {xw[3 * (size_t)p], xw[3 * (size_t)p + 1], xw[3 * (size_t)p + 2]};
  float o[3] = {P[0], P[1], P[2]};
  const int r = refVertex[p];
  if (r >= 0) ess_correct_point(sim3 + 8 * (size_t)r, sim3Out + 8 * (size_t)r, P, o);
  xwOut[3 * (size_t)p] = o[0]; xwOut[3 * (size_t)p + 1] = o[1]; xwOut[3 * (size_t)p + 2] = o[2];
}

__global__ __launch_bounds__(kEssThreads) void k_ess_correct_table(const double* sim3, const double* sim3Out, int nPoints,
                                                                   MapPointsDevice t, const int32_t* slot, const int32_t* refVertex) {
  const int p = blockIdx.x * kEssThreads + threadIdx.x;
  if (p >= nPoints) return;
  const int r = refVertex[p];
  if (r < 0) return;
  float4* rec = t.rec + 2 * (size_t)slot[p];
  const float P[3] = {rec->x, rec->y, rec->z};
  float o[3];
  ess_correct_point(sim3 + 8 * (size_t)r, sim3Out + 8 * (size_t)r, P, o);
  rec->x = o[0]; rec->y = o[1]; rec->z = o[2];
}

__global__ __launch_bounds__(kEssThreads) void k_ess_read_positions(MapPointsDevice t, const int32_t* slot, int n, float* xw) {
  const int p = blockIdx.x * kEssThreads + threadIdx.x;
  if (p >= n) return;
  const float4 r = t.rec[2 * (size_t)slot[p]];
  xw[3 * (size_t)p] = r.x; xw[3 * (size_t)p + 1] = r.y; xw[3 * (size_t)p + 2] = r.z;
}

inline int blocks_of(size_t n) { return (int)((n + kEssThreads - 1) / kEssThreads); }

}  // namespace

void launch_ess_measure(hipStream_t s, const EssArgs& a) {
  if (a.nEdges > 0) hipLaunchKernelGGL(k_ess_measure, dim3(blocks_of((size_t)a.nEdges)), dim3(kEssThreads), 0, s, a);
}

void launch_ess_linearise(hipStream_t s, const EssArgs& a, int cur) {
  hipLaunchKernelGGL(k_ess_linearise, dim3(blocks_of((size_t)a.nActive)), dim3(kEssThreads), 0, s, a, cur);
  hipLaunchKernelGGL(k_ess_assemble, dim3(a.blocksA), dim3(kEssLanes), 0, s, a);
  hipLaunchKernelGGL(k_ess_record, dim3(1), dim3(kEssLanes), 0, s, a, 0.0, 1);
}

void launch_ess_solve(hipStream_t s, const EssArgs& a) {
  hipLaunchKernelGGL(k_ess_load, dim3(blocks_of(49 * (size_t)a.blocksL)), dim3(kEssThreads), 0, s, a, 0.0);
  hipLaunchKernelGGL(k_ess_factor, dim3(1), dim3(kEssFactorThreads), 0, s, a, 0, 0);
}

void launch_ess_trial(hipStream_t s, const EssArgs& a, int cur, double lambda) {
  hipLaunchKernelGGL(k_ess_load, dim3(blocks_of(49 * (size_t)a.blocksL)), dim3(kEssThreads), 0, s, a, lambda);
  hipLaunchKernelGGL(k_ess_factor, dim3(1), dim3(kEssFactorThreads), 0, s, a, cur, 1);
  hipLaunchKernelGGL(k_ess_trial_edges, dim3(blocks_of((size_t)a.nActive)), dim3(kEssThreads), 0, s, a, cur);
  hipLaunchKernelGGL(k_ess_record, dim3(1), dim3(kEssLanes), 0, s, a, lambda, 0);
}

void launch_ess_correct_points(hipStream_t s, const double* sim3, const double* sim3Out, int nPoints, const float* xw,
                               const int32_t* refVertex, float* xwOut, const MapPointsDevice* table, const int32_t* slot) {
  if (nPoints <= 0) return;
  if (table)
    hipLaunchKernelGGL(k_ess_correct_table, dim3(blocks_of((size_t)nPoints)), dim3(kEssThreads), 0, s, sim3, sim3Out, nPoints, *table, slot,
                       refVertex);
  else
    hipLaunchKernelGGL(k_ess_correct_points, dim3(blocks_of((size_t)nPoints)), dim3(kEssThreads), 0, s, sim3, sim3Out, nPoints, xw,
                       refVertex, xwOut);
}

void launch_ess_read_positions(hipStream_t s, const MapPointsDevice& table, const int32_t* slot, int n, float* xw) {
  if (n > 0) hipLaunchKernelGGL(k_ess_read_positions, dim3(blocks_of((size_t)n)), dim3(kEssThreads), 0, s, table, slot, n, xw);
}

}  // namespace orbfe
