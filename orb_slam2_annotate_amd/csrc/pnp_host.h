// pnp_host.h -- the host side of orbfe_pnp_* (pnp.hip) that needs no device: the argument checks, the layout of a call
// (candidate records, the candidate of every hypothesis or Refine record, the mask-word offsets, the index lists of the
// records), the scan that lists the Refine records, and the pure host function orbfe_pnp_sets_from_draws.  Plain C++ without a
// HIP include, so a stand-alone program can run exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include <vector>

#include "pnp_math.h"

namespace orbfe {

constexpr int kPnpHostMaxCandidates = 4096;

inline bool pnp_offsets_ok(const int32_t* off, int K, int total) {
  if (off[0] != 0 || off[K] != total) return false;
  for (int k = 0; k < K; k++)
    if (off[k + 1] < off[k]) return false;
  return true;
}

// what the ransac and the refine call share.  item_off = hyp_off or rec_off, I items in all.  NULL when fine
inline const char* pnp_check_common(int K, int N, int I, const int32_t* point_off, const float* p3d, const float* p2d,
                                    const float* max_err2, const float* cam, const int32_t* item_off, const void* items,
                                    const int32_t* n_inliers, const uint8_t* status, const float* pose, const int32_t* word_off,
                                    const uint32_t* mask_words) {
  if (K < 0 || K > kPnpHostMaxCandidates) return "n_candidates outside [0, 4096]";
  if (N < 0 || I < 0) return "negative count";
  if (!point_off || !item_off || !word_off) return "NULL offsets";
  if (K > 0 && !cam) return "NULL camera";
  if (N > 0 && (!p3d || !p2d || !max_err2)) return "NULL point array";
  if (I > 0 && (!items || !n_inliers || !status || !pose || !mask_words)) return "NULL hypothesis or record array";
  if (!pnp_offsets_ok(point_off, K, N)) return "point_off is not monotone from 0 to n_points";
  if (!pnp_offsets_ok(item_off, K, I)) return "hyp_off / rec_off is not monotone from 0 to the total";
  size_t words = 0;
  for (int k = 0; k < K; k++) {
    for (int i = 0; i < 4; i++)
      if (!isfinite(cam[4 * k + i])) return "camera entry is not finite";
    const int n = point_off[k + 1] - point_off[k], items_k = item_off[k + 1] - item_off[k];
    if (items_k > 0 && n < 4) return "a candidate with fewer than 4 correspondences has hypotheses or records";
    words += (size_t)items_k * (size_t)((n + 31) / 32);
    if (words > (size_t)INT32_MAX) return "more than 2^31 - 1 mask words";
  }
  return nullptr;
}

inline const char* pnp_check_sets(int K, const int32_t* point_off, const int32_t* hyp_off, const int32_t* sets) {
  for (int k = 0; k < K; k++) {
    const int n = point_off[k + 1] - point_off[k];
    for (int h = hyp_off[k]; h < hyp_off[k + 1]; h++) {
      const int32_t* s = sets + 4 * (size_t)h;
      for (int i = 0; i < 4; i++) {
        if (s[i] < 0 || s[i] >= n) return "set index outside [0, n_k)";
        for (int j = 0; j < i; j++)
          if (s[i] == s[j]) return "set repeats an index";
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
  if (K < 0 || K > kPnpHostMaxCandidates) return "n_candidates outside [0, 4096]";
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
  itemCand->clear();
  word_off[0] = 0;
  for (int k = 0; k < K; k++) {
    PnpCandidate c;
    c.point0 = point_off[k]; c.nPoints = point_off[k + 1] - point_off[k];
    c.hyp0 = item_off[k];
    c.word0 = word_off[k]; c.words = (c.nPoints + 31) / 32;
    c.K = PnpCamera{cam[4 * k], cam[4 * k + 1], cam[4 * k + 2], cam[4 * k + 3]};
    cands->push_back(c);
    const int items = item_off[k + 1] - item_off[k];
    itemCand->insert(itemCand->end(), (size_t)items, k);
    word_off[k + 1] = word_off[k] + items * c.words;
  }
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

// The selection without replacement of PnPsolver::iterate (:201-214) for H hypotheses over n correspondences: draws[4 h + i]
// is the value RandomInt(0, size - 1) returned with size = n - i, the index INTO vAvailableIndices; the entry taken leaves
// the list by swap-with-back and pop.  The list starts as 0 .. n-1 for every hypothesis (:201).  The random stream itself is
// the caller's.  false: n < 4, a NULL array or a draw outside [0, n - 1 - i]; sets is then unspecified.
inline bool pnp_sets_from_draws(int n, int H, const int32_t* draws, int32_t* sets) {
  if (H == 0) return n >= 0;
  if (n < 4 || H < 0 || !draws || !sets) return false;
  std::vector<int32_t> avail((size_t)n);
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int h = 0; h < H; h++) {
    int32_t at[4] = {0, 0, 0, 0};
    int size = n, done = 0;
    bool ok = true;
    for (int i = 0; i < 4; i++) {
      const int32_t r = draws[4 * (size_t)h + i];
      ok = r >= 0 && r <= size - 1;
      if (!ok) break;
      sets[4 * (size_t)h + i] = avail[r];  // :208
      avail[r] = avail[size - 1];          // :212
      size--;                              // :213
      at[done++] = r;
    }
    // the list of the next hypothesis is whole again (:201): undo in reverse, each slot back to what it held
    for (int i = done - 1; i >= 0; i--) {
      avail[at[i]] = sets[4 * (size_t)h + i];
    }
    if (!ok) return false;
  }
  return true;
}

}  // namespace orbfe
