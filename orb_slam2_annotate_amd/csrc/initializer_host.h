// initializer_host.h -- the host side of orbfe_initializer_ransac* and orbfe_initializer_reconstruct* (initializer.hip) that
// needs no device: the argument checks, the problem records of the layouts and the two pure host functions
// orbfe_initializer_normalize / orbfe_initializer_sets_from_draws.  What the three RANSAC solvers share (offsets check, set
// predicate, layout walk, selection without replacement) is ransac_host.h; recon_layout keeps its own loop, because there
// the item counts are not given but follow from model_kind and hyp_off is an output.  Plain C++ without a HIP include, so
// tests/cpp/initializer_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "initializer_math.h"
#include "initializer_reconstruct_math.h"
#include "ransac_host.h"

namespace orbfe {

constexpr int kInitHostMaxSets = 1 << 24;  // 2 waves per set: the launch stays far below 2^31 waves

// NULL when the arguments are fine, else what is wrong with them.  N pairs and H sets in all.
inline const char* init_check(int K, int N, int H, const int32_t* pair_off, const float* pairs, const double* T1, const double* T2,
                              const float* sigma, const int32_t* hyp_off, const int32_t* sets, const double* score,
                              const uint8_t* status, const int32_t* n_inliers, const double* model, const double* h12,
                              const uint32_t* mask_words, const int32_t* word_off) {
  if (K < 0 || K > kRansacMaxOwners) return "n_problems outside [0, 4096]";
  if (N < 0 || H < 0) return "negative count";
  if (H > kInitHostMaxSets) return "more than 2^24 sets";
  if (!pair_off || !hyp_off || !word_off) return "NULL offsets";
  if (K > 0 && (!T1 || !T2 || !sigma)) return "NULL T1 / T2 / sigma";
  if (N > 0 && !pairs) return "NULL pair array";
  if (H > 0 && (!sets || !score || !status || !n_inliers || !model || !h12 || !mask_words)) return "NULL set or output array";
  if (!offsets_ok(pair_off, K, N)) return "pair_off is not monotone from 0 to n_pairs";
  if (!offsets_ok(hyp_off, K, H)) return "hyp_off is not monotone from 0 to n_sets";
  size_t words = 0;
  for (int k = 0; k < K; k++) {
    for (int i = 0; i < 4; i++)
      if (!isfinite(T1[4 * k + i]) || !isfinite(T2[4 * k + i])) return "T1 / T2 entry is not finite";
    if (!isfinite(sigma[k]) || !(sigma[k] > 0.0f)) return "sigma is not positive and finite";
    const int n = pair_off[k + 1] - pair_off[k], h0 = hyp_off[k], h1 = hyp_off[k + 1];
    if (h1 > h0 && n < 8) return "a problem with fewer than 8 pairs has sets";
    for (int h = h0; h < h1; h++) {
      const int32_t* s = sets + 8 * (size_t)h;
      for (int j = 0; j < 8; j++) {
        if (set_index_outside(s, j, n)) return "set index outside [0, n_k)";
        if (set_index_repeats(s, j)) return "set repeats an index";
      }
    }
    if (!add_mask_words(&words, 2, h1 - h0, n)) return kTooManyMaskWords;  // an H and an F mask per set
  }
  return nullptr;
}

// the arguments have passed init_check: word_off [K + 1], the problem records and the problem of every set
inline void init_layout(int K, const int32_t* pair_off, const int32_t* hyp_off, const double* T1, const double* T2,
                        const float* sigma, int32_t* word_off, std::vector<InitProblem>* probs, std::vector<int32_t>* hypProb) {
  probs->clear();
  layout_walk(K, pair_off, hyp_off, 2, word_off, hypProb, [&](int k, int n, int words) {  // an H and an F mask per set
    InitProblem p = {};
    p.pair0 = pair_off[k]; p.nPairs = n;
    p.hyp0 = hyp_off[k];
    p.word0 = word_off[k]; p.words = words;
    p.sigma = sigma[k];
    for (int i = 0; i < 4; i++) { p.T1[i] = T1[4 * k + i]; p.T2[i] = T2[4 * k + i]; }
    probs->push_back(p);
  });
}

// orbfe_initializer_reconstruct*: NULL when the arguments are fine, else what is wrong with them.  N pairs and W inlier words
// in all; G / slots receive the totals of hypotheses and of per-(hypothesis, pair) records when the offsets are fine.
inline const char* recon_check(int K, int N, int W, const int32_t* pair_off, const float* pairs, const int32_t* model_kind,
                               const double* model, const float* K4, const float* sigma, const uint32_t* inlier_words,
                               const int32_t* in_word_off, const int32_t* hyp_off, const int32_t* slot_off, const double* R,
                               const double* t, const int32_t* n_good, const double* cos_sel, const uint8_t* hyp_status,
                               const double* x3d, const uint8_t* pair_flags, const uint8_t* problem_status,
                               const int32_t* n_inliers) {
  if (K < 0 || K > kRansacMaxOwners) return "n_problems outside [0, 4096]";
  if (N < 0 || W < 0 || N > INT32_MAX - 31) return "count negative or above 2^31 - 32";
  if (!pair_off || !in_word_off || !hyp_off || !slot_off) return "NULL offsets";
  if (K > 0 && (!model_kind || !model || !K4 || !sigma || !R || !t || !n_good || !cos_sel || !hyp_status || !problem_status ||
                !n_inliers || !x3d || !pair_flags))
    return "NULL problem or output array";
  if (N > 0 && !pairs) return "NULL pair array";
  if (W > 0 && !inlier_words) return "NULL inlier words";
  if (!offsets_ok(pair_off, K, N)) return "pair_off is not monotone from 0 to n_pairs";
  if (!offsets_ok(in_word_off, K, W)) return "in_word_off is not monotone from 0 to n_words";
  size_t slots = 0;
  for (int k = 0; k < K; k++) {
    if (model_kind[k] != kInitH && model_kind[k] != kInitF) return "model_kind is neither ORBFE_INIT_MODEL_H nor _F";
    for (int i = 0; i < 9; i++)
      if (!isfinite(model[9 * (size_t)k + i])) return "model entry is not finite";
    for (int i = 0; i < 4; i++)
      if (!isfinite(K4[4 * (size_t)k + i])) return "K4 entry is not finite";
    if (K4[4 * (size_t)k] == 0.0f || K4[4 * (size_t)k + 1] == 0.0f) return "fx or fy is 0";
    if (!isfinite(sigma[k]) || !(sigma[k] > 0.0f)) return "sigma is not positive and finite";
    const int n = pair_off[k + 1] - pair_off[k];
    if (in_word_off[k + 1] - in_word_off[k] != (n + 31) / 32) return "a problem does not have ceil(n_k / 32) inlier words";
    slots += (size_t)recon_hyps(model_kind[k]) * (size_t)n;
    if (slots > (size_t)INT32_MAX) return "more than 2^31 - 1 (hypothesis, pair) records";
  }
  return nullptr;
}

// the arguments have passed recon_check: hyp_off / slot_off [K + 1], the problem records and the problem of every hypothesis
inline void recon_layout(int K, const int32_t* pair_off, const int32_t* model_kind, const double* model, const float* K4,
                         const float* sigma, const int32_t* in_word_off, int32_t* hyp_off, int32_t* slot_off,
                         std::vector<ReconProblem>* probs, std::vector<int32_t>* hypProb) {
  probs->clear();
  hypProb->clear();
  hyp_off[0] = 0;
  slot_off[0] = 0;
  for (int k = 0; k < K; k++) {
    ReconProblem p = {};
    p.pair0 = pair_off[k]; p.nPairs = pair_off[k + 1] - pair_off[k];
    p.word0 = in_word_off[k];
    p.hyp0 = hyp_off[k]; p.nHyp = recon_hyps(model_kind[k]);
    p.slot0 = slot_off[k];
    p.kind = model_kind[k];
    p.sigma = sigma[k];
    for (int i = 0; i < 4; i++) p.K[i] = K4[4 * (size_t)k + i];
    for (int i = 0; i < 9; i++) p.model[i] = model[9 * (size_t)k + i];
    probs->push_back(p);
    hypProb->insert(hypProb->end(), (size_t)p.nHyp, k);
    hyp_off[k + 1] = hyp_off[k] + p.nHyp;
    slot_off[k + 1] = slot_off[k] + p.nHyp * p.nPairs;
  }
}

// Initializer::Normalize (src/Initializer.cc:852-904) over n keys (x y interleaved) -> T = sX sY meanX meanY, in binary64
// with sequential sums in index order (the reference sums in float).  false: n <= 0 or a NULL array.
inline bool init_normalize(int n, const float* xy, double T[4]) {
  if (n <= 0 || !xy || !T) return false;
  double meanX = 0.0, meanY = 0.0;
  for (int i = 0; i < n; i++) { meanX += (double)xy[2 * (size_t)i]; meanY += (double)xy[2 * (size_t)i + 1]; }  // :861-865
  meanX = meanX / n; meanY = meanY / n;  // :867-868
  double meanDevX = 0.0, meanDevY = 0.0;
  for (int i = 0; i < n; i++) {  // :876-883
    meanDevX += fabs((double)xy[2 * (size_t)i] - meanX);
    meanDevY += fabs((double)xy[2 * (size_t)i + 1] - meanY);
  }
  meanDevX = meanDevX / n; meanDevY = meanDevY / n;  // :885-886
  T[0] = 1.0 / meanDevX; T[1] = 1.0 / meanDevY;       // :889-890
  T[2] = meanX; T[3] = meanY;
  return true;
}

// Initializer::Initialize's selection without replacement (ransac_host.h, S = 8); false: n < 8 with sets, a NULL array or a
// draw outside [0, n - j)
inline bool init_sets_from_draws(int n, int H, const int32_t* draws, int32_t* sets) { return sets_from_draws<8>(n, H, draws, sets); }

}  // namespace orbfe
