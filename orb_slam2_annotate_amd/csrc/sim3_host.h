// sim3_host.h -- the host side of orbfe_sim3_ransac* (sim3.hip) that needs no device: the argument checks, the candidate
// record of the layout and the two pure host functions orbfe_sim3_triples_from_draws / orbfe_sim3_max_iterations.  What the
// three RANSAC solvers share (offsets check, set predicate, layout walk, selection without replacement) is ransac_host.h.
// Plain C++ without a HIP include, so tests/cpp/sim3_host_san.cpp runs exactly this code under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "ransac_host.h"
#include "sim3_math.h"

namespace orbfe {

// NULL when the arguments are fine, else what is wrong with them.  N pairs and H hypotheses in all.
inline const char* sim3_check(int K, int N, int H, const int32_t* pair_off, const float* x3dc1, const float* x3dc2,
                              const float* max_err1, const float* max_err2, const float* cam1, const float* cam2,
                              const int32_t* hyp_off, const int32_t* triples, const int32_t* n_inliers, const uint8_t* status,
                              const float* sim3, const uint32_t* mask_words, const int32_t* word_off) {
  if (K < 0 || K > kRansacMaxOwners) return "n_candidates outside [0, 4096]";
  if (N < 0 || H < 0) return "negative count";
  if (!pair_off || !hyp_off || !word_off) return "NULL offsets";
  if (K > 0 && (!cam1 || !cam2)) return "NULL camera";
  if (N > 0 && (!x3dc1 || !x3dc2 || !max_err1 || !max_err2)) return "NULL pair array";
  if (H > 0 && (!triples || !n_inliers || !status || !sim3 || !mask_words)) return "NULL hypothesis array";
  if (!offsets_ok(pair_off, K, N)) return "pair_off is not monotone from 0 to n_pairs";
  if (!offsets_ok(hyp_off, K, H)) return "hyp_off is not monotone from 0 to n_hypotheses";
  size_t words = 0;
  for (int k = 0; k < K; k++) {
    for (int i = 0; i < 4; i++)
      if (!isfinite(cam1[4 * k + i]) || !isfinite(cam2[4 * k + i])) return "camera entry is not finite";
    const int n = pair_off[k + 1] - pair_off[k], h0 = hyp_off[k], h1 = hyp_off[k + 1];
    if (h1 > h0 && n < 3) return "a candidate with fewer than 3 pairs has hypotheses";
    for (int h = h0; h < h1; h++) {
      const int32_t* t = triples + 3 * (size_t)h;  // all three ranges before any repeat
      for (int i = 0; i < 3; i++)
        if (set_index_outside(t, i, n)) return "triple index outside [0, n_k)";
      if (set_index_repeats(t, 1) || set_index_repeats(t, 2)) return "triple repeats an index";
    }
    if (!add_mask_words(&words, 1, h1 - h0, n)) return kTooManyMaskWords;
  }
  return nullptr;
}

// the arguments have passed sim3_check: word_off [K + 1], the candidate records and the candidate of every hypothesis
inline void sim3_layout(int K, const int32_t* pair_off, const int32_t* hyp_off, const float* cam1, const float* cam2,
                        int32_t* word_off, std::vector<Sim3Candidate>* cands, std::vector<int32_t>* hypCand) {
  cands->clear();
  layout_walk(K, pair_off, hyp_off, 1, word_off, hypCand, [&](int k, int n, int words) {
    Sim3Candidate c;
    c.pair0 = pair_off[k]; c.nPairs = n;
    c.hyp0 = hyp_off[k];
    c.word0 = word_off[k]; c.words = words;
    c.K1 = Sim3Camera{cam1[4 * k], cam1[4 * k + 1], cam1[4 * k + 2], cam1[4 * k + 3]};
    c.K2 = Sim3Camera{cam2[4 * k], cam2[4 * k + 1], cam2[4 * k + 2], cam2[4 * k + 3]};
    cands->push_back(c);
  });
}

// Sim3Solver::iterate's selection without replacement (ransac_host.h, S = 3); false: n < 3 or a draw outside [0, n - 1 - i]
inline bool sim3_triples_from_draws(int n, int H, const int32_t* draws, int32_t* triples) {
  return sets_from_draws<3>(n, H, draws, triples);
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
