// sim3_host.h -- the host side of orbfe_sim3_ransac* (sim3.hip) that needs no device: the argument checks, the layout of a
// call (candidate records, the candidate of every hypothesis, the mask-word offsets) and the two pure host functions
// orbfe_sim3_triples_from_draws / orbfe_sim3_max_iterations.  Plain C++ without a HIP include, so
// tests/cpp/sim3_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "sim3_math.h"

namespace orbfe {

constexpr int kSim3HostMaxCandidates = 4096;

inline bool sim3_offsets_ok(const int32_t* off, int K, int total) {
  if (off[0] != 0 || off[K] != total) return false;
  for (int k = 0; k < K; k++)
    if (off[k + 1] < off[k]) return false;
  return true;
}

// NULL when the arguments are fine, else what is wrong with them.  N pairs and H hypotheses in all.
inline const char* sim3_check(int K, int N, int H, const int32_t* pair_off, const float* x3dc1, const float* x3dc2,
                              const float* max_err1, const float* max_err2, const float* cam1, const float* cam2,
                              const int32_t* hyp_off, const int32_t* triples, const int32_t* n_inliers, const uint8_t* status,
                              const float* sim3, const uint32_t* mask_words, const int32_t* word_off) {
  if (K < 0 || K > kSim3HostMaxCandidates) return "n_candidates outside [0, 4096]";
  if (N < 0 || H < 0) return "negative count";
  if (!pair_off || !hyp_off || !word_off) return "NULL offsets";
  if (K > 0 && (!cam1 || !cam2)) return "NULL camera";
  if (N > 0 && (!x3dc1 || !x3dc2 || !max_err1 || !max_err2)) return "NULL pair array";
  if (H > 0 && (!triples || !n_inliers || !status || !sim3 || !mask_words)) return "NULL hypothesis array";
  if (!sim3_offsets_ok(pair_off, K, N)) return "pair_off is not monotone from 0 to n_pairs";
  if (!sim3_offsets_ok(hyp_off, K, H)) return "hyp_off is not monotone from 0 to n_hypotheses";
  size_t words = 0;
  for (int k = 0; k < K; k++) {
    for (int i = 0; i < 4; i++)
      if (!isfinite(cam1[4 * k + i]) || !isfinite(cam2[4 * k + i])) return "camera entry is not finite";
    const int n = pair_off[k + 1] - pair_off[k], h0 = hyp_off[k], h1 = hyp_off[k + 1];
    if (h1 > h0 && n < 3) return "a candidate with fewer than 3 pairs has hypotheses";
    for (int h = h0; h < h1; h++) {
      const int32_t a = triples[3 * (size_t)h], b = triples[3 * (size_t)h + 1], c = triples[3 * (size_t)h + 2];
      if (a < 0 || a >= n || b < 0 || b >= n || c < 0 || c >= n) return "triple index outside [0, n_k)";
      if (a == b || a == c || b == c) return "triple repeats an index";
    }
    words += (size_t)(h1 - h0) * (size_t)((n + 31) / 32);
    if (words > (size_t)INT32_MAX) return "more than 2^31 - 1 mask words";
  }
  return nullptr;
}

// the arguments have passed sim3_check: word_off [K + 1], the candidate records and the candidate of every hypothesis
inline void sim3_layout(int K, const int32_t* pair_off, const int32_t* hyp_off, const float* cam1, const float* cam2,
                        int32_t* word_off, std::vector<Sim3Candidate>* cands, std::vector<int32_t>* hypCand) {
  cands->clear();
  hypCand->clear();
  word_off[0] = 0;
  for (int k = 0; k < K; k++) {
    Sim3Candidate c;
    c.pair0 = pair_off[k]; c.nPairs = pair_off[k + 1] - pair_off[k];
    c.hyp0 = hyp_off[k];
    c.word0 = word_off[k]; c.words = (c.nPairs + 31) / 32;
    c.K1 = Sim3Camera{cam1[4 * k], cam1[4 * k + 1], cam1[4 * k + 2], cam1[4 * k + 3]};
    c.K2 = Sim3Camera{cam2[4 * k], cam2[4 * k + 1], cam2[4 * k + 2], cam2[4 * k + 3]};
    cands->push_back(c);
    const int h = hyp_off[k + 1] - hyp_off[k];
    hypCand->insert(hypCand->end(), (size_t)h, k);
    word_off[k + 1] = word_off[k] + h * c.words;
  }
}

// The selection without replacement of Sim3Solver::iterate (src/Sim3Solver.cc:173-187) for H hypotheses over n pairs:
// draws[3 h + i] is the value RandomInt(0, size - 1) returned with size = n - i, the index INTO the list of still available
// pairs; the pair taken leaves the list by swap-with-back and pop.  The list starts as 0 .. n-1 for every hypothesis
// (:173).  The random stream itself (DUtils::Random::RandomInt over rand()) is the caller's: it is not restated here.
// false: n < 3 or a draw outside [0, n - 1 - i]; triples is then unspecified.
inline bool sim3_triples_from_draws(int n, int H, const int32_t* draws, int32_t* triples) {
  if (H == 0) return n >= 0;
  if (n < 3 || H < 0 || !draws || !triples) return false;
  std::vector<int32_t> avail((size_t)n);
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int h = 0; h < H; h++) {
    int32_t at[3] = {0, 0, 0};
    int size = n, done = 0;
    bool ok = true;
    for (int i = 0; i < 3 && ok; i++) {
      const int32_t r = draws[3 * (size_t)h + i];
      ok = r >= 0 && r <= size - 1;
      if (!ok) break;
      triples[3 * (size_t)h + i] = avail[r];  // :180
      avail[r] = avail[size - 1];             // :185
      size--;                                 // :186
      at[done++] = r;
    }
    for (int i = 0; i < done; i++) avail[at[i]] = at[i];  // the list of the next hypothesis is whole again (:173)
    if (!ok) return false;
  }
  return true;
}

// Sim3Solver::SetRansacParameters (:118-142): the number of iterations mRansacMaxIts becomes, with the reference's float
// epsilon and double pow / log / ceil.  n < min_inliers is answered before the formula -- epsilon > 1 makes the reference's
// expression log of a negative number, NaN, whose conversion to int is undefined, and iterate() returns at :156 without ever
// reading it -- with 1, the least max(1, .) can give.  For an epsilon so small that 1 - epsilon^3 rounds to 1 the quotient is
// log(1 - prob) / +0 = -infinity, whose conversion to int is undefined in the reference as well (INT_MIN on x86, hence 1):
// it is below 1 and gives 1 here.  A quotient that is not below max_its gives max_its.
inline int sim3_max_iterations(int n, double prob, int min_inliers, int max_its) {
  if (n < min_inliers || n <= 0) return 1;
  if (min_inliers == n) return 1;  // :134
  const float epsilon = (float)min_inliers / n;  // :129
  const double its = ceil(log(1 - prob) / log(1 - pow((double)epsilon, 3)));  // :137
  if (!(its < (double)max_its)) return max_its > 1 ? max_its : 1;  // :139
  return its > 1.0 ? (int)its : 1;
}

}  // namespace orbfe
