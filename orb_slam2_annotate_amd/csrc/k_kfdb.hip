// k_kfdb.hip -- the scored set of KeyFrameDatabase::DetectLoopCandidates / DetectRelocalizationCandidates
// (src/KeyFrameDatabase.cc:95-163, :228-291) over BowVectors resident in HBM as one CSR, Q queries per call.
//
// The reference walks an inverted file: for every word of the query, every key frame listed under it gets a mark and a
// counter.  The inverted file is a transposition of the stored BowVectors, so the same numbers come out of the
// forward direction, which is a plain streaming read:
//   k_kfdb_count    one wave per stored key frame: its lanes take the key frame's words 64 at a time and look each up in
//                   the query's ascending word list (a copy in LDS); ballot + popcount is mnLoopWords / mnRelocWords,
//                   and the first hit is the SMALLEST shared word, because the stored words ascend too
//   k_kfdb_exclude  zeroes the counter of the (query, key frame) pairs of spConnectedKeyFrames (:116)
//   k_kfdb_select   one workgroup per query: maxCommonWords, minCommonWords = (int)(max * 0.8f), and the key frames with
//                   more shared words than that, compacted in slot order by ballot prefixes (no atomics)
//   k_kfdb_score    one wave per (query, survivor): L1Scoring::score (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68).
//                   The sum runs over the shared words in ascending order in ONE double accumulator -- the lanes find
//                   the shared words and form the terms, then the terms are added one by one in lane order.  The wave
//                   also ranks its survivor among the query's by (smallest shared word, slot), which is the order the
//                   reference's list holds them in, and writes its result at that rank.
// Nothing here adds floating-point numbers in an order that depends on scheduling.
#include "kfdb_kernels.h"

namespace orbfe {
namespace {

constexpr int kSlotsPerBlock = 16;  // k_kfdb_count: 4 waves x 4 key frames share one LDS copy of the query

// position of w in the ascending list q[0..n), or -1
__device__ __forceinline__ int find_word(const uint32_t* q, int n, uint32_t w) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (q[mid] < w) lo = mid + 1; else hi = mid;
  }
  return (lo < n && q[lo] == w) ? lo : -1;
}

extern __shared__ uint32_t s_query[];  // the query's words (kLds forms)

// the calling workgroup's query words: copied to LDS (kLds) or left in global memory
template <bool kLds>
__device__ __forceinline__ const uint32_t* stage_query(const uint32_t* qw, int qn) {
  if constexpr (kLds) {
    for (int i = threadIdx.x; i < qn; i += blockDim.x) s_query[i] = qw[i];
    __syncthreads();
    return s_query;
  } else {
    return qw;
  }
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_kfdb_count(KfdbStore st, KfdbQueries p) {
  const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qoff = p.qOff[q], qn = p.qOff[q + 1] - qoff;
  const uint32_t* qw = stage_query<kLds>(p.qWords + qoff, qn);
  const int s0 = blockIdx.x * kSlotsPerBlock;
  const int s1 = s0 + kSlotsPerBlock < st.nSlots ? s0 + kSlotsPerBlock : st.nSlots;
  for (int s = s0 + wave; s < s1; s += 4) {
    const KfdbSlot sl = st.slots[s];
    const uint32_t* sw = st.words + sl.off;
    uint32_t common = 0, first = 0;
    for (uint32_t base = 0; base < sl.n; base += 64) {
      const uint32_t i = base + lane;
      const uint32_t w = i < sl.n ? sw[i] : 0u;
      const bool hit = i < sl.n && find_word(qw, qn, w) >= 0;
      const unsigned long long m = __ballot(hit);
      if (m && !common) first = (uint32_t)__shfl((int)w, __ffsll((long long)m) - 1);
      common += (uint32_t)__popcll(m);
    }
    if (lane == 0) {
      p.common[(size_t)q * st.nSlots + s] = common;
      p.minWord[(size_t)q * st.nSlots + s] = first;
    }
  }
}

__global__ __launch_bounds__(256) void k_kfdb_exclude(KfdbQueries p, int nQueries, int nSlots) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= p.nExcl) return;
  int q = 0;  // the query whose range holds entry i (Q is small: a scan)
  while (q + 1 < nQueries && p.exclOff[q + 1] <= i) q++;
  const uint32_t s = p.exclSlots[i];
  if (s < (uint32_t)nSlots) p.common[(size_t)q * nSlots + s] = 0;
}

__global__ __launch_bounds__(256) void k_kfdb_select(KfdbQueries p, int nSlots) {
  __shared__ uint32_t red[4];
  __shared__ int waveTot[4];
  const int q = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const uint32_t* common = p.common + (size_t)q * nSlots;
  uint32_t mx = 0;
  for (int s = tid; s < nSlots; s += 256) mx = common[s] > mx ? common[s] : mx;
  for (int d = 32; d > 0; d >>= 1) {
    const uint32_t o = (uint32_t)__shfl_xor((int)mx, d);
    mx = o > mx ? o : mx;
  }
  if (lane == 0) red[wave] = mx;
  __syncthreads();
  for (int w = 0; w < 4; w++) mx = red[w] > mx ? red[w] : mx;
  // int minCommonWords = maxCommonWords*0.8f (:141, :265): a float product, truncated
  const int minCommon = (int)((float)(int)mx * 0.8f);
  uint32_t* surv = p.surv + (size_t)q * nSlots;
  int run = 0;
  for (int base = 0; base < nSlots; base += 256) {
    const int s = base + tid;
    const bool keep = s < nSlots && (int)common[s] > minCommon;  // minCommon >= 0: a key frame sharing no word never stays
    const unsigned long long m = __ballot(keep);
    __syncthreads();  // the previous round's waveTot has been read
    if (lane == 0) waveTot[wave] = __popcll(m);
    __syncthreads();
    int o = run + __popcll(m & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) o += waveTot[w];
    run += waveTot[0] + waveTot[1] + waveTot[2] + waveTot[3];
    if (keep) surv[o] = (uint32_t)s;
  }
  if (tid == 0) p.nSurv[q] = run;
}

// score(v1 = the query, v2 = the stored key frame), the same value in every lane of the calling wave
__device__ __forceinline__ double wave_l1_score(const uint32_t* qw, int qn, const double* qv, const uint32_t* sw,
                                                const double* sv, uint32_t sn, int lane) {
  double score = 0;
  for (uint32_t base = 0; base < sn; base += 64) {
    const uint32_t i = base + lane;
    const int pos = i < sn ? find_word(qw, qn, sw[i]) : -1;
    double term = 0;
    if (pos >= 0) {
      const double vi = qv[pos], wi = sv[i];
      term = fabs(vi - wi) - fabs(vi) - fabs(wi);
    }
    unsigned long long m = __ballot(pos >= 0);
    while (m) {  // ascending word order = lane order; wave-uniform loop
      const int l = __ffsll((long long)m) - 1;
      m &= m - 1;
      score += __shfl(term, l);
    }
  }
  return -score / 2.0;
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_kfdb_score(KfdbStore st, KfdbQueries p) {
  const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int ns = p.nSurv[q];
  if (blockIdx.x * 4 >= ns) return;  // the whole workgroup: before the LDS copy and its barrier
  const int qoff = p.qOff[q], qn = p.qOff[q + 1] - qoff;
  const uint32_t* qw = stage_query<kLds>(p.qWords + qoff, qn);
  const uint32_t* surv = p.surv + (size_t)q * st.nSlots;
  const uint32_t* minWord = p.minWord + (size_t)q * st.nSlots;
  for (int i = blockIdx.x * 4 + wave; i < ns; i += gridDim.x * 4) {
    const uint32_t s = surv[i];
    const KfdbSlot sl = st.slots[s];
    const double score = wave_l1_score(qw, qn, p.qValues + qoff, st.words + sl.off, st.values + sl.off, sl.n, lane);
    // rank among the query's survivors by (smallest shared word, slot)
    const unsigned long long key = ((unsigned long long)minWord[s] << 32) | s;
    int rank = 0;
    for (int base = 0; base < ns; base += 64) {
      const int j = base + lane;
      bool before = false;
      if (j < ns) {
        const uint32_t sj = surv[j];
        before = (((unsigned long long)minWord[sj] << 32) | sj) < key;
      }
      rank += __popcll(__ballot(before));
    }
    if (lane == 0 && rank < p.capacity) {
      const size_t o = (size_t)q * p.capacity + rank;
      p.outSlot[o] = s;
      p.outCommon[o] = (int32_t)p.common[(size_t)q * st.nSlots + s];
      p.outScore[o] = (float)score;  // float si = mpVoc->score(...) (:154, :279)
    }
  }
}

template <bool kLds>
__global__ __launch_bounds__(256) void k_kfdb_score_named(KfdbStore st, KfdbQueries p, const uint32_t* slotIds, int nIds,
                                                          double* scores) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int qn = p.qOff[1] - p.qOff[0];
  const uint32_t* qw = stage_query<kLds>(p.qWords + p.qOff[0], qn);
  const int i = blockIdx.x * 4 + wave;
  if (i >= nIds) return;
  const uint32_t s = slotIds[i];
  if (s >= (uint32_t)st.nSlots) return;
  const KfdbSlot sl = st.slots[s];
  const double score = wave_l1_score(qw, qn, p.qValues + p.qOff[0], st.words + sl.off, st.values + sl.off, sl.n, lane);
  if (lane == 0) scores[i] = score;
}

}  // namespace

void launch_kfdb_query(hipStream_t s, const KfdbStore& st, const KfdbQueries& q, int nQueries) {
  // the host side calls with 1 <= nQueries <= 65535 (gridDim.y) and at least one slot
  const bool lds = q.maxWords <= kKfdbLdsWords;
  const size_t shm = lds ? (size_t)(q.maxWords > 0 ? q.maxWords : 1) * 4 : 0;
  const dim3 gc((st.nSlots + kSlotsPerBlock - 1) / kSlotsPerBlock, nQueries);
  if (lds) hipLaunchKernelGGL(k_kfdb_count<true>, gc, dim3(256), shm, s, st, q);
  else hipLaunchKernelGGL(k_kfdb_count<false>, gc, dim3(256), 0, s, st, q);
  if (q.nExcl > 0) hipLaunchKernelGGL(k_kfdb_exclude, dim3((q.nExcl + 255) / 256), dim3(256), 0, s, q, nQueries, st.nSlots);
  hipLaunchKernelGGL(k_kfdb_select, dim3(nQueries), dim3(256), 0, s, q, st.nSlots);
  int gx = (st.nSlots + 3) / 4;
  if (gx > 256) gx = 256;
  if (lds) hipLaunchKernelGGL(k_kfdb_score<true>, dim3(gx, nQueries), dim3(256), shm, s, st, q);
  else hipLaunchKernelGGL(k_kfdb_score<false>, dim3(gx, nQueries), dim3(256), 0, s, st, q);
}

void launch_kfdb_score(hipStream_t s, const KfdbStore& st, const KfdbQueries& q, const uint32_t* slotIds, int nIds,
                       double* scores) {
  if (nIds <= 0) return;
  const bool lds = q.maxWords <= kKfdbLdsWords;
  const size_t shm = lds ? (size_t)(q.maxWords > 0 ? q.maxWords : 1) * 4 : 0;
  if (lds) hipLaunchKernelGGL(k_kfdb_score_named<true>, dim3((nIds + 3) / 4), dim3(256), shm, s, st, q, slotIds, nIds, scores);
  else hipLaunchKernelGGL(k_kfdb_score_named<false>, dim3((nIds + 3) / 4), dim3(256), 0, s, st, q, slotIds, nIds, scores);
}

}  // namespace orbfe
