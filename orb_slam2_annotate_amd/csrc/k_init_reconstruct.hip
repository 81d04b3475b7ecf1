// k_init_reconstruct.hip -- ReconstructH / ReconstructF (src/Initializer.cc:536-824) up to their order-dependent tails, ONE
// launch: one WORKGROUP of 256 lanes per (problem, hypothesis) -- 8 per H problem, 4 per F problem.
//   prologue: every lane computes the hypothesis's (R, t) from the problem's model and K (initializer_reconstruct_math.h:
//             the 3 x 3 Jacobi SVD and Faugeras' / DecomposeE's formulas, a few hundred flops) rather than reading it from
//             another launch; the values are the same in every lane, so every branch on them is uniform.
//   check:    lane l handles pairs l, l + 256, ... of its problem; a pair whose inlier bit is set runs CheckRT's body
//             (recon_pair: the 4 x 4 null vector, the parallax, two depth and two reprojection tests) and stores its point,
//             its flags and its selection key (the cosine of a counted pair as an order-preserving 64-bit integer, else
//             kReconNoKey).  The other pairs store zeros, so every output byte is written.
//   counts:   nGood, the number of keys and the problem's inlier count are INTEGER sums: a shuffle tree inside each wave,
//             four LDS slots, one barrier.  No floating-point sum crosses a lane and there is no atomic anywhere.
//   select:   the cosine at index min(50, n_sel - 1) of the ascending order (:1018-1023) by bisection on the key: 64 passes,
//             most significant bit first, each counting the keys <= the probe over the workgroup.  Exact, O(64 n), LDS of 20
//             integers whatever n.  A lane re-reads only the keys it wrote itself.
// The device takes no acos: it returns the cosine, and the replay turns it into degrees.
// Every output byte is a function of the hypothesis's own inputs, so two runs, and the multi and the single form, give
// identical bytes; the CPU build of the header performs the same operations in the same order.
#include <hip/hip_runtime.h>

#include "initializer_kernels.h"

namespace orbfe {

namespace {

// the sum of v over the workgroup, in every lane; slots = 4 ints of LDS that no earlier sum still reads
__device__ inline int block_sum(int v, int* slots) {
  v += __shfl_xor(v, 32);
  v += __shfl_xor(v, 16);
  v += __shfl_xor(v, 8);
  v += __shfl_xor(v, 4);
  v += __shfl_xor(v, 2);
  v += __shfl_xor(v, 1);
  if ((threadIdx.x & 63) == 0) slots[threadIdx.x >> 6] = v;
  __syncthreads();
  return slots[0] + slots[1] + slots[2] + slots[3];
}

__global__ __launch_bounds__(kReconThreads) void k_init_reconstruct(ReconArgs A) {
  __shared__ int red[5][4];
  const int g = (int)blockIdx.x;  // (the launch has exactly nHyp workgroups)
  const int k = A.hypProb[g];
  const ReconProblem* P = A.probs + k;
  const int hi = g - P->hyp0, n = P->nPairs, pair0 = P->pair0, kind = P->kind;
  const float K4[4] = {P->K[0], P->K[1], P->K[2], P->K[3]};
  double model[9], R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; i++) model[i] = P->model[i];
  const bool deg = recon_motion(kind, model, K4, hi, R, t);
  ReconCam cam;
  recon_camera(K4, R, t, P->sigma, &cam);

  const size_t slot = (size_t)P->slot0 + (size_t)hi * (size_t)n;
  const uint32_t* words = A.words + P->word0;
  int good = 0, sel = 0, inl = 0;
  for (int i = (int)threadIdx.x; i < n; i += kReconThreads) {
    const bool in = ((words[i >> 5] >> (i & 31)) & 1u) != 0;
    inl += in ? 1 : 0;
    double X[3] = {0.0, 0.0, 0.0}, cosP = 0.0;
    int f = 0;
    if (in && !deg) {
      const float4 q = *reinterpret_cast<const float4*>(A.pairs + 4 * (size_t)(pair0 + i));
      const float p[4] = {q.x, q.y, q.z, q.w};
      f = recon_pair(cam, p, X, &cosP);
    }
    const uint64_t key = recon_sel_key(f, cosP);
    A.keys[slot + (size_t)i] = key;
    A.pairFlags[slot + (size_t)i] = (uint8_t)f;
    A.x3d[3 * (slot + (size_t)i)] = X[0];
    A.x3d[3 * (slot + (size_t)i) + 1] = X[1];
    A.x3d[3 * (slot + (size_t)i) + 2] = X[2];
    good += (f & kReconCounted) ? 1 : 0;
    sel += key != kReconNoKey ? 1 : 0;
  }
  good = block_sum(good, red[0]);
  sel = block_sum(sel, red[1]);
  inl = block_sum(inl, red[2]);

  double c = 0.0;
  if (sel > 0) {  // (uniform: a workgroup sum)
    const int rank = sel - 1 < kReconSelIndex ? sel - 1 : kReconSelIndex;  // :1022
    uint64_t prefix = 0;
    for (int b = 63; b >= 0; b--) {
      const uint64_t probe = recon_bisect_probe(prefix, b);
      int cnt = 0;
      for (int i = (int)threadIdx.x; i < n; i += kReconThreads) cnt += A.keys[slot + (size_t)i] <= probe ? 1 : 0;
      // slots alternate: a wave that runs ahead writes the slots of pass b - 1 only after every wave has passed the barrier
      // of pass b, hence after it has read those of pass b + 1
      cnt = block_sum(cnt, red[3 + (b & 1)]);
      if (cnt < rank + 1) prefix |= (uint64_t)1 << b;
    }
    c = recon_unkey(prefix);
  }
  if (threadIdx.x == 0) {
#pragma unroll
    for (int i = 0; i < 9; i++) A.R[9 * (size_t)g + i] = R[i];
#pragma unroll
    for (int i = 0; i < 3; i++) A.t[3 * (size_t)g + i] = t[i];
    A.nGood[g] = good;
    A.cosSel[g] = c;
    A.hypStatus[g] = (uint8_t)(good != sel ? kReconNonfinite : kReconOk);
    if (hi == 0) {
      A.nInliers[k] = inl;
      A.problemStatus[k] = (uint8_t)(deg ? kReconDegenerate : kReconProblemOk);
    }
  }
}

}  // namespace

void launch_init_reconstruct(hipStream_t s, const ReconArgs& a) {
  if (a.nHyp <= 0) return;
  hipLaunchKernelGGL(k_init_reconstruct, dim3(a.nHyp), dim3(kReconThreads), 0, s, a);
}

}  // namespace orbfe
