// pnp_host.h -- the host side of orbfe_pnp_* (pnp.hip) that needs no device: the argument checks, the candidate record of
// the layout, the index lists of the Refine records, the scan that lists those records, and the pure host function
// orbfe_pnp_sets_from_draws.  What the three RANSAC solvers share (offsets check, set predicate, layout walk, selection
// without replacement) is ransac_host.h.  Plain C++ without a HIP include, so a stand-alone program can run exactly this
// code under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pnp_math.h"
#include "ransac_host.h"

namespace orbfe {

// what the ransac and the refine call share.  item_off = hyp_off or rec_off, I items in all.  NULL when fine
inline const char* pnp_check_common(int K, int N, int I, const int32_t* point_off, const float* p3d, const float* p2d,
                                    const float* max_err2, const float* cam, const int32_t* item_off, const void* items,
                                    const int32_t* n_inliers, const uint8_t* status, const float* pose, const int32_t* word_off,
                                    const uint32_t* mask_words) {
  if (K < 0 || K > kRansacMaxOwners) return "n_candidates outside [0, 4096]";
  if (N < 0 || I < 0) return "negative count";
  if (!point_off || !item_off || !word_off) return "NULL offsets";
  if (K > 0 && !cam) return "NULL camera";
  if (N > 0 && (!p3d || !p2d || !max_err2)) return "NULL point array";
  if (I > 0 && (!items || !n_inliers || !status || !pose || !mask_words)) return "NULL hypothesis or record array";
  if (!offsets_ok(point_off, K, N)) return "point_off is not monotone from 0 to n_points";
  if (!offsets_ok(item_off, K, I)) return "hyp_off / rec_off is not monotone from 0 to the total";
  size_t words = 0;
  for (int k = 0; k < K; k++) {
    for (int i = 0; i < 4; i++)
      if (!isfinite(cam[4 * k + i])) return "camera entry is not finite";
    const int n = point_off[k + 1] - point_off[k], items_k = item_off[k + 1] - item_off[k];
    if (items_k > 0 && n < 4) return "a candidate with fewer than 4 correspondences has hypotheses or records";
    if (!add_mask_words(&words, 1, items_k, n)) return kTooManyMaskWords;
  }
  return nullptr;
}

inline const char* pnp_check_sets(int K, const int32_t* point_off, const int32_t* hyp_off, const int32_t* sets) {
  for (int k = 0; k < K; k++) {
    const int n = point_off[k + 1] - point_off[k];
    for (int h = hyp_off[k]; h < hyp_off[k + 1]; h++) {
      const int32_t* s = sets + 4 * (size_t)h;
      for (int i = 0; i < 4; i++) {
        if (set_index_outside(s, i, n)) return "set index outside [0, n_k)";
        if (set_index_repeats(s, i)) return "set repeats an index";
      }
    }
  }
  return nullptr;
}

// the records' masks: ceil(n_k / 32) words each, candidate after candidate
inline const char* pnp_check_masks(int K, const int32_t* point_off, const int32_t* rec_off, const uint32_t* rec_masks) {
  size_t w0 = 0, total = 0;
  for (int k = 0; k < K; k++) {
    const int n = point_off[k + 1] - point_off[k], words = (n + 31) / 32;
    for (int r = rec_off[k]; r < rec_off[k + 1]; r++, w0 += (size_t)words) {
      int bits = 0;
      for (int w = 0; w < words; w++) {
        const uint32_t m = rec_masks[w0 + w];
        if (w == words - 1 && (n & 31) && (m >> (n & 31))) return "record mask has bits at or beyond n_k";
        bits += __builtin_popcount(m);
      }
      if (bits < 4) return "record mask with fewer than 4 bits";
      total += (size_t)bits;  // pnp_compact's index list is addressed with int32
      if (total > (size_t)INT32_MAX) return "more than 2^31 - 1 record correspondences";
    }
  }
  return nullptr;
}

// what orbfe_pnp_solve_multi takes besides the arguments of the ransac call.  NULL when fine
inline const char* pnp_check_solve(int K, int H, const int32_t* min_inliers, const int32_t* rec_off, const int32_t* rec_hyp,
                                   const int32_t* rec_n_inliers, const uint8_t* rec_status, const float* rec_pose,
                                   const int32_t* rec_word_off, const uint32_t* rec_mask_words) {
  if (K < 0 || K > kRansacMaxOwners) return "n_candidates outside [0, 4096]";
  if (!rec_off || !rec_word_off) return "NULL record offsets";
  if (K > 0 && !min_inliers) return "NULL min_inliers";
  if (H > 0 && (!rec_hyp || !rec_n_inliers || !rec_status || !rec_pose || !rec_mask_words)) return "NULL record array";
  for (int k = 0; k < K; k++)
    if (min_inliers[k] < 4) return "min_inliers below the minimal set of 4";
  return nullptr;
}

// the arguments have passed the checks: word_off [K + 1], the candidate records and the candidate of every item
inline void pnp_layout(int K, const int32_t* point_off, const int32_t* item_off, const float* cam, int32_t* word_off,
                       std::vector<PnpCandidate>* cands, std::vector<int32_t>* itemCand) {
  cands->clear();
  layout_walk(K, point_off, item_off, 1, word_off, itemCand, [&](int k, int n, int words) {
    PnpCandidate c;
    c.point0 = point_off[k]; c.nPoints = n;
    c.hyp0 = item_off[k];
    c.word0 = word_off[k]; c.words = words;
    c.K = PnpCamera{cam[4 * k], cam[4 * k + 1], cam[4 * k + 2], cam[4 * k + 3]};
    cands->push_back(c);
  });
}

// the set bits of every record's mask, ascending: idx and idxOff [R + 1] (Refine's vIndices, :277-286)
inline void pnp_compact(int K, const int32_t* point_off, const int32_t* rec_off, const uint32_t* rec_masks,
                        std::vector<int32_t>* idxOff, std::vector<int32_t>* idx) {
  idxOff->assign(1, 0);
  idx->clear();
  size_t w0 = 0;
  for (int k = 0; k < K; k++) {
    const int n = point_off[k + 1] - point_off[k], words = (n + 31) / 32;
    for (int r = rec_off[k]; r < rec_off[k + 1]; r++, w0 += (size_t)words) {
      for (int i = 0; i < n; i++)
        if (rec_masks[w0 + (size_t)(i >> 5)] >> (i & 31) & 1u) idx->push_back(i);
      idxOff->push_back((int32_t)idx->size());
    }
  }
}

// The distinct Refine problems of every solver (iterate(), :222-239): Refine() runs on mvbBestInliers, which changes only
// where a hypothesis has count >= min_inliers_k AND count > every earlier such count (mnBestInliers starts at 0), and it is a
// pure function of that set.  rec_off [K + 1], rec_hyp = those hypotheses (global indices), ascending.
inline void pnp_scan_records(int K, const int32_t* hyp_off, const int32_t* n_inliers, const int32_t* min_inliers,
                             int32_t* rec_off, std::vector<int32_t>* rec_hyp) {
  rec_hyp->clear();
  rec_off[0] = 0;
  for (int k = 0; k < K; k++) {
    int best = 0;
    for (int h = hyp_off[k]; h < hyp_off[k + 1]; h++)
      if (n_inliers[h] >= min_inliers[k] && n_inliers[h] > best) {
        best = n_inliers[h];
        rec_hyp->push_back(h);
      }
    rec_off[k + 1] = (int32_t)rec_hyp->size();
  }
}

// PnPsolver::iterate's selection without replacement (ransac_host.h, S = 4); false: n < 4, a NULL array or a draw outside
// [0, n - 1 - i]
inline bool pnp_sets_from_draws(int n, int H, const int32_t* draws, int32_t* sets) { return sets_from_draws<4>(n, H, draws, sets); }

}  // namespace orbfe
