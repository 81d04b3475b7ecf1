// k_pnp.hip -- the two launches of a PnPsolver call (src/PnPsolver.cc:178-354).
//
// k_pnp_ransac: every RANSAC hypothesis of every candidate (:199-220: compute_pose on four correspondences, then CheckInliers
// over all correspondences of the candidate) as one launch: one WAVE per hypothesis, four per workgroup.  The 4-point EPnP of
// pnp_math.h is one instruction stream per wave (lane 0 runs it; a wave costs what one lane costs) on a PnpWork in the wave's
// slice of LDS -- every array the algebra indexes at run time -- and the pose reaches the other lanes through __shfl.  Lane l
// then tests correspondences l, l + 64, ...; each trip's __ballot is stored by lanes 0 and 1 as two uint32 mask words
// (correspondence i at bit i & 31 of word i >> 5); the count is the sum of the ballots' popcounts.
//
// k_pnp_refine: every Refine problem (:275-320: compute_pose on the n correspondences of a best inlier set, then CheckInliers)
// as one launch: one 256-lane workgroup per record.  Lane l owns points l, l + 256, ... of the record's index list and keeps
// per-lane partial sums; every n-dependent sum (the centroid, PW0^T PW0, the 78 unique entries of M^T M, and per solution
// the camera-point centroid, ABt and the reprojection error) is combined in a fixed tree: an xor butterfly inside each wave
// (all lanes end with the same bits, addition being commutative), then ((w0 + w1) + w2) + w3 over the four waves through
// LDS.  Thread 0 runs the fixed-size algebra on the PnpWork in LDS; all lanes run CheckInliers over the candidate's
// correspondences.
//
// No atomics, no cross-workgroup reduction: every output byte is a function of the item's own inputs, so two runs give
// identical bytes.  All indices come from arrays the host has checked (pnp_host.h).
#include <hip/hip_runtime.h>

#include "pnp_kernels.h"

namespace orbfe {

namespace {

// the four correspondences of a hypothesis, read where they lie
struct SetPoints {
  const float* p3d;
  const float* p2d;
  const int32_t* set;
  int point0;
  __device__ int n() const { return 4; }
  __device__ void get(int i, double pw[3], double uv[2]) const {
    const size_t p = (size_t)(point0 + set[i]);
    pw[0] = (double)p3d[3 * p]; pw[1] = (double)p3d[3 * p + 1]; pw[2] = (double)p3d[3 * p + 2];
    uv[0] = (double)p2d[2 * p]; uv[1] = (double)p2d[2 * p + 1];
  }
};

// CheckInliers of one wave over the correspondences base + lane of each of its trips; `stride` = correspondences per trip of
// the whole group (64 for a wave alone, 256 for a workgroup), `first` = the wave's offset inside a trip
__device__ inline int check_inliers(const PnpArgs& A, const PnpCandidate& C, const double R[9], const double t[3], bool bad, int lane,
                                    int first, int stride, uint32_t* words) {
  int count = 0;
  for (int base = first; base < C.nPoints; base += stride) {
    const int i = base + lane;
    bool in = false;
    if (!bad && i < C.nPoints) {
      const size_t p = (size_t)(C.point0 + i);
      const float P[3] = {A.p3d[3 * p], A.p3d[3 * p + 1], A.p3d[3 * p + 2]};
      const float q[2] = {A.p2d[2 * p], A.p2d[2 * p + 1]};
      in = pnp_is_inlier(R, t, C.K, P, q, A.maxErr2[p]);
    }
    const unsigned long long m = __ballot(in);
    count += __popcll(m);
    const int w = (base >> 5) + lane;  // lanes 0, 1: the two words of this trip
    if (lane < 2 && w < C.words) words[w] = lane ? (uint32_t)(m >> 32) : (uint32_t)m;
  }
  return count;
}

__device__ inline void store_result(const PnpArgs& A, int item, int count, bool bad, const double R[9], const double t[3]) {
  A.nInliers[item] = count;
  A.status[item] = (uint8_t)(bad ? kPnpNonfinite : kPnpOk);
  float* o = A.pose + 12 * (size_t)item;  // what mBestTcw holds: the binary64 values rounded once
#pragma unroll
  for (int i = 0; i < 9; i++) o[i] = (float)R[i];
#pragma unroll
  for (int i = 0; i < 3; i++) o[9 + i] = (float)t[i];
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_ransac(PnpArgs A) {
  __shared__ PnpWork work[kPnpWavesPerBlock];
  const int lane = (int)(threadIdx.x & 63);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int h = (int)blockIdx.x * kPnpWavesPerBlock + wave;
  if (h >= A.nItems) return;  // (a whole wave; the kernel has no workgroup barrier)
  const PnpCandidate C = A.cands[A.itemCand[h]];
  double R[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, t[3] = {0.0, 0.0, 0.0};
  if (lane == 0) {
    const SetPoints P = {A.p3d, A.p2d, A.sets + 4 * (size_t)h, C.point0};
    pnp_compute_pose(P, C.K, &work[wave], R, t);
  }
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = __shfl(R[i], 0);
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = __shfl(t[i], 0);
  const bool bad = pnp_nonfinite(R, t);
  uint32_t* words = A.words + (size_t)C.word0 + (size_t)(h - C.hyp0) * (size_t)C.words;
  const int count = check_inliers(A, C, R, t, bad, lane, 0, 64, words);
  if (lane == 0) store_result(A, h, count, bad, R, t);
}

// the fixed tree of the head of the file on NV per-lane values at once; every thread returns with the totals in x.
// red: [kPnpWavesPerBlock][NV]
template <int NV>
__device__ inline void block_sum(double (&x)[NV], double* red, int lane, int wave) {
#pragma unroll
  for (int k = 0; k < NV; k++) {
    double v = x[k];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    x[k] = v;
  }
  __syncthreads();  // red is free again: everybody has read the previous totals
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < NV; k++) red[wave * NV + k] = x[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < NV; k++) x[k] = ((red[k] + red[NV + k]) + red[2 * NV + k]) + red[3 * NV + k];
}

__global__ __launch_bounds__(kPnpThreads) void k_pnp_refine(PnpArgs A) {
  __shared__ PnpWork W;
  __shared__ double red[kPnpWavesPerBlock * 78];
  __shared__ int cnt[kPnpWavesPerBlock];
  const int tid = (int)threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int r = (int)blockIdx.x;  // (the grid is exactly nItems workgroups)
  const PnpCandidate C = A.cands[A.itemCand[r]];
  const int32_t* idx = A.idx + A.idxOff[r];
  const int n = A.idxOff[r + 1] - A.idxOff[r];
  auto get = [&](int i, double pw[3], double uv[2]) {
    const size_t p = (size_t)(C.point0 + idx[i]);
    pw[0] = (double)A.p3d[3 * p]; pw[1] = (double)A.p3d[3 * p + 1]; pw[2] = (double)A.p3d[3 * p + 2];
    uv[0] = (double)A.p2d[2 * p]; uv[1] = (double)A.p2d[2 * p + 1];
  };
  double pw[3], uv[2], as[4];

  // choose_control_points
  double c0[3];
  {
    double s[3] = {0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kPnpThreads) {
      get(i, pw, uv);
      s[0] += pw[0]; s[1] += pw[1]; s[2] += pw[2];
    }
    block_sum<3>(s, red, lane, wave);
#pragma unroll
    for (int j = 0; j < 3; j++) c0[j] = s[j] / n;
  }
  {
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int i = tid; i < n; i += kPnpThreads) {
      get(i, pw, uv);
      const double d0 = pw[0] - c0[0], d1 = pw[1] - c0[1], d2 = pw[2] - c0[2];
      s[0] += d0 * d0; s[1] += d0 * d1; s[2] += d0 * d2; s[3] += d1 * d1; s[4] += d1 * d2; s[5] += d2 * d2;
    }
    block_sum<6>(s, red, lane, wave);
    if (tid == 0) {
      const double cov[9] = {s[0], s[1], s[2], s[1], s[3], s[4], s[2], s[4], s[5]};
      pnp_control_points(c0, cov, n, W.cws);
      pnp_cc_inv(W.cws, W.ci);
    }
    __syncthreads();
  }
  double ci[9];
#pragma unroll
  for (int j = 0; j < 9; j++) ci[j] = W.ci[j];

  if (n == 4) {  // (the whole workgroup) the canonical null-space basis of the minimal problem, as k_pnp_ransac
    if (tid == 0) {
      double M1[12], M2[12];
      for (int i = 0; i < 4; i++) {
        get(i, pw, uv);
        pnp_alphas(ci, c0, pw, as);
        pnp_fill_M(as, uv[0], uv[1], C.K, M1, M2);
#pragma unroll
        for (int c = 0; c < 12; c++) { W.a[8 * c + 2 * i] = M1[c]; W.a[8 * c + 2 * i + 1] = M2[c]; }
      }
      pnp_null4(&W);
      pnp_all_betas(&W);
    }
  } else {  // M^T M: the upper triangle, row-major
    double s[78];
#pragma unroll
    for (int k = 0; k < 78; k++) s[k] = 0.0;
    for (int i = tid; i < n; i += kPnpThreads) {
      double M1[12], M2[12];
      get(i, pw, uv);
      pnp_alphas(ci, c0, pw, as);
      pnp_fill_M(as, uv[0], uv[1], C.K, M1, M2);
      int k = 0;
#pragma unroll
      for (int a = 0; a < 12; a++)
#pragma unroll
        for (int b = a; b < 12; b++) s[k++] += M1[a] * M1[b] + M2[a] * M2[b];
    }
    block_sum<78>(s, red, lane, wave);
    if (tid == 0) {
      int k = 0;
#pragma unroll
      for (int a = 0; a < 12; a++)
#pragma unroll
        for (int b = a; b < 12; b++) { W.a[12 * a + b] = s[k]; W.a[12 * b + a] = s[k]; k++; }
      pnp_eig12(&W);
      pnp_all_betas(&W);
    }
  }

  // the three compute_R_and_t and the choice of N (:580-595)
  double R[9], t[3], best = 0.0;
  for (int which = 1; which <= 3; which++) {
    if (tid == 0) {
      double pc[3];
      pnp_ccs(&W, which);
      get(0, pw, uv);
      pnp_alphas(ci, c0, pw, as);
      pnp_pc(as, W.ccs, pc);
      pnp_solve_for_sign(&W, pc);
    }
    __syncthreads();
    double ccs[4][3];
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
      for (int b = 0; b < 3; b++) ccs[a][b] = W.ccs[a][b];
    double pc[3], pc0[3];
    {
      double s[3] = {0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += kPnpThreads) {
        get(i, pw, uv);
        pnp_alphas(ci, c0, pw, as);
        pnp_pc(as, ccs, pc);
        s[0] += pc[0]; s[1] += pc[1]; s[2] += pc[2];
      }
      block_sum<3>(s, red, lane, wave);
#pragma unroll
      for (int j = 0; j < 3; j++) pc0[j] = s[j] / n;
    }
    double Rn[9], tn[3];
    {
      double s[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      for (int i = tid; i < n; i += kPnpThreads) {
        get(i, pw, uv);
        pnp_alphas(ci, c0, pw, as);
        pnp_pc(as, ccs, pc);
#pragma unroll
        for (int j = 0; j < 3; j++) {
          s[3 * j] += (pc[j] - pc0[j]) * (pw[0] - c0[0]);
          s[3 * j + 1] += (pc[j] - pc0[j]) * (pw[1] - c0[1]);
          s[3 * j + 2] += (pc[j] - pc0[j]) * (pw[2] - c0[2]);
        }
      }
      block_sum<9>(s, red, lane, wave);
      pnp_estimate_R_and_t(pc0, c0, s, Rn, tn);  // (every thread, on the same bits)
    }
    double e[1] = {0.0};
    for (int i = tid; i < n; i += kPnpThreads) {
      get(i, pw, uv);
      e[0] += pnp_reprojection_term(Rn, tn, C.K, pw, uv[0], uv[1]);
    }
    block_sum<1>(e, red, lane, wave);  // (its barriers also keep W.ccs until every thread has finished with it)
    const double err = e[0] / n;
    if (which == 1 || err < best) {  // :591-593: N = 1 first, strict <
      best = err;
#pragma unroll
      for (int j = 0; j < 9; j++) R[j] = Rn[j];
#pragma unroll
      for (int j = 0; j < 3; j++) t[j] = tn[j];
    }
  }

  const bool bad = pnp_nonfinite(R, t);
  uint32_t* words = A.words + (size_t)C.word0 + (size_t)(r - C.hyp0) * (size_t)C.words;
  const int count = check_inliers(A, C, R, t, bad, lane, 64 * wave, kPnpThreads, words);
  if (lane == 0) cnt[wave] = count;
  __syncthreads();
  if (tid == 0) store_result(A, r, cnt[0] + cnt[1] + cnt[2] + cnt[3], bad, R, t);
}

}  // namespace

void launch_pnp_ransac(hipStream_t s, const PnpArgs& a) {
  if (a.nItems <= 0) return;
  const int blocks = (a.nItems + kPnpWavesPerBlock - 1) / kPnpWavesPerBlock;
  hipLaunchKernelGGL(k_pnp_ransac, dim3(blocks), dim3(kPnpThreads), 0, s, a);
}

void launch_pnp_refine(hipStream_t s, const PnpArgs& a) {
  if (a.nItems <= 0) return;
  hipLaunchKernelGGL(k_pnp_refine, dim3(a.nItems), dim3(kPnpThreads), 0, s, a);
}

}  // namespace orbfe
