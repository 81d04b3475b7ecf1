// k_initializer.hip -- every RANSAC hypothesis of Initializer::FindHomography and FindFundamental (src/Initializer.cc:141-255)
// of every problem as one launch: one WAVE per (set, model), four per workgroup; the model is wave-uniform.
//   solve: lane l owns row l of the stacked matrix [A; V] of initializer_math.h (lanes 0-15 the rows of A -- for F rows 8-15
//          are zero --, lanes 16-24 the rows of V, the others a zero row) as 9 doubles.  A column-pair rotation sums three
//          products over lanes 0-15 by an xor butterfly (8, 4, 2, 1) and a broadcast of lane 0, then every lane rotates its
//          own row.  All column indices are compile-time and the 36 pairs of a sweep are unrolled, so nothing is indexed at
//          run time; the picked column of V is read from lanes 16-24.  What follows the null vector (the 3 x 3 products, the
//          inverse, F's rank-2 step) is wave-uniform: every lane computes it.
//   check: lane l tests pairs l, l + 64, ... and adds their score terms in ascending order; each trip's __ballot is stored by
//          lanes 0 and 1 as two uint32 mask words (pair i at bit i & 31 of word i >> 5).  The score is the xor butterfly
//          32, 16, ..., 1 over the 64 partial sums.  A hypothesis whose score or model is not finite has its words rewritten to
//          zero by the lanes that wrote them.
// No atomics, no LDS, no scratch.  Every output byte is a function of the hypothesis's inputs alone, so two runs give identical
// bytes.
#include <hip/hip_runtime.h>

#include "initializer_kernels.h"

namespace orbfe {

namespace {

// lane `l`'s x in every lane, as a wave-uniform (scalar) value: what follows it branches without divergence
__device__ inline double lane_value(double x, int l) {
  return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l), __builtin_amdgcn_readlane(__double2loint(x), l));
}

struct InitWaveLanes {
  static constexpr int kOwned = 1;
  __device__ double sum_a(const double* part) const {
    double x = part[0];
    x += __shfl_xor(x, 8);
    x += __shfl_xor(x, 4);
    x += __shfl_xor(x, 2);
    x += __shfl_xor(x, 1);
    return lane_value(x, 0);
  }
  __device__ double pick(const double* vals, int row) const { return lane_value(vals[0], row); }
};

__device__ inline double sum64(double x) {
  x += __shfl_xor(x, 32);
  x += __shfl_xor(x, 16);
  x += __shfl_xor(x, 8);
  x += __shfl_xor(x, 4);
  x += __shfl_xor(x, 2);
  x += __shfl_xor(x, 1);
  return lane_value(x, 0);
}

__global__ __launch_bounds__(kInitThreads) void k_initializer(InitArgs A) {
  const int lane = (int)(threadIdx.x & 63);
  const int w = (int)blockIdx.x * kInitWavesPerBlock + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (w >= 2 * A.nHyp) return;  // (a whole wave)
  const int h = w >> 1, model = w & 1;
  const InitProblem* P = A.probs + A.hypProb[h];
  const int pair0 = P->pair0, nPairs = P->nPairs, nWords = P->words;
  double T1[4], T2[4];
#pragma unroll
  for (int i = 0; i < 4; i++) { T1[i] = P->T1[i]; T2[i] = P->T2[i]; }

  double m[1][9], nv[9];
  {
    const int j = init_row_pair(model, lane);
    float p[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    if (j >= 0) {
      const float4 q = *reinterpret_cast<const float4*>(A.pairs + 4 * (size_t)(pair0 + A.sets[8 * (size_t)h + j]));
      p[0] = q.x; p[1] = q.y; p[2] = q.z; p[3] = q.w;
    }
    init_fill_row(model, lane, p, T1, T2, m[0]);
  }
  const InitWaveLanes ln;
  init_null_vector(ln, m, nv);
  double M[9], H12[9];
#pragma unroll
  for (int i = 0; i < 9; i++) H12[i] = 0.0;
  if (model == kInitH) init_model_h(nv, T1, T2, M, H12);
  else init_model_f(nv, T1, T2, M);

  const double sigma = (double)P->sigma;
  const double invSigmaSquare = 1.0 / (sigma * sigma);  // :380
  uint32_t* words = A.words + (size_t)P->word0 + ((size_t)(h - P->hyp0) * 2 + (size_t)model) * (size_t)nWords;
  double part = 0.0;
  int count = 0;
  for (int base = 0; base < nPairs; base += 64) {
    const int i = base + lane;
    bool in = false;
    if (i < nPairs) {
      const float4 q = *reinterpret_cast<const float4*>(A.pairs + 4 * (size_t)(pair0 + i));
      const float p[4] = {q.x, q.y, q.z, q.w};
      in = model == kInitH ? init_check_h(M, H12, invSigmaSquare, p, &part) : init_check_f(M, invSigmaSquare, p, &part);
    }
    const unsigned long long b = __ballot(in);
    count += __popcll(b);
    const int wd = (base >> 5) + lane;  // lanes 0, 1: the two words of this trip
    if (lane < 2 && wd < nWords) words[wd] = lane ? (uint32_t)(b >> 32) : (uint32_t)b;
  }
  const double score = sum64(part);
  const bool bad = init_nonfinite(score, M, H12);
  if (bad) {
    count = 0;
    for (int base = 0; base < nPairs; base += 64) {
      const int wd = (base >> 5) + lane;
      if (lane < 2 && wd < nWords) words[wd] = 0u;
    }
  }
  if (lane == 0) {
    const size_t g = 2 * (size_t)h + (size_t)model;
    A.score[g] = score;
    A.nInliers[g] = count;
    A.status[g] = (uint8_t)(bad ? kInitNonfinite : kInitOk);
#pragma unroll
    for (int i = 0; i < 9; i++) A.model[9 * g + i] = M[i];
    if (model == kInitH) {
#pragma unroll
      for (int i = 0; i < 9; i++) A.h12[9 * (size_t)h + i] = H12[i];
    }
  }
}

}  // namespace

void launch_initializer(hipStream_t s, const InitArgs& a) {
  if (a.nHyp <= 0) return;
  const int waves = 2 * a.nHyp;
  const int blocks = (waves + kInitWavesPerBlock - 1) / kInitWavesPerBlock;
  hipLaunchKernelGGL(k_initializer, dim3(blocks), dim3(kInitThreads), 0, s, a);
}

}  // namespace orbfe
