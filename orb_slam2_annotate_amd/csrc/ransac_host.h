// ransac_host.h -- what the host layers of the three RANSAC solvers (sim3_host.h, pnp_host.h, initializer_host.h) share: the
// offsets check, the minimal-set predicate, the selection without replacement, the walk that lays a call out and the guard
// on the number of mask words.  An "owner" is a candidate (Sim3Solver, PnPsolver) or a problem (Initializer); its "items" are
// its hypotheses, sets or Refine records.  Plain C++ without a HIP include, like the headers it serves.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace orbfe {

constexpr int kRansacMaxOwners = 4096;  // candidates or problems of one call
constexpr const char* kTooManyMaskWords = "more than 2^31 - 1 mask words";

// off [K + 1] is monotone from 0 to total
inline bool offsets_ok(const int32_t* off, int K, int total) {
  if (off[0] != 0 || off[K] != total) return false;
  for (int k = 0; k < K; k++)
    if (off[k + 1] < off[k]) return false;
  return true;
}

// The minimal-set predicate by position, so that a check names the faults of a set in the order it always did:
// s[i] is outside [0, n) / s[i] repeats one of s[0 .. i)
inline bool set_index_outside(const int32_t* s, int i, int n) { return s[i] < 0 || s[i] >= n; }
inline bool set_index_repeats(const int32_t* s, int i) {
  for (int j = 0; j < i; j++)
    if (s[j] == s[i]) return true;
  return false;
}

// adds the mask words of an owner with n entries -- factor * items * ceil(n / 32) -- to *words; false once word_off, which
// is int32, cannot address them
inline bool add_mask_words(size_t* words, int factor, int items, int n) {
  *words += (size_t)factor * (size_t)items * (size_t)((n + 31) / 32);
  return *words <= (size_t)INT32_MAX;
}

// The layout of a checked call of K owners: word_off [K + 1] with factor * items_k * ceil(n_k / 32) words per owner, the
// owner of every item, and record(k, n_k, words_k) once per owner, in order, with word_off[k] already final, for the
// solver's own record.
template <typename Record>
inline void layout_walk(int K, const int32_t* entry_off, const int32_t* item_off, int factor, int32_t* word_off,
                        std::vector<int32_t>* owner, Record&& record) {
  owner->clear();
  word_off[0] = 0;
  for (int k = 0; k < K; k++) {
    const int n = entry_off[k + 1] - entry_off[k], items = item_off[k + 1] - item_off[k], words = (n + 31) / 32;
    record(k, n, words);
    owner->insert(owner->end(), (size_t)items, k);
    word_off[k + 1] = word_off[k] + factor * items * words;
  }
}

// The selection without replacement of Sim3Solver::iterate (src/Sim3Solver.cc:173-187, S = 3), PnPsolver::iterate
// (src/PnPsolver.cc:201-214, S = 4) and Initializer::Initialize (src/Initializer.cc:93-108, S = 8) for H sets over n entries:
// draws[S h + i] is the value RandomInt(0, size - 1) returned with size = n - i, the index INTO the list of still available
// entries; the entry taken leaves the list by swap-with-back and pop.  The list starts as 0 .. n-1 for every set.  The
// random stream itself (DUtils::Random::RandomInt over rand()) is the caller's: it is not restated here.
// false: n < S with sets to make, a NULL array or a draw outside [0, n - 1 - i]; sets is then unspecified.
template <int S>
inline bool sets_from_draws(int n, int H, const int32_t* draws, int32_t* sets) {
  if (H == 0) return n >= 0;
  if (n < S || H < 0 || !draws || !sets) return false;
  std::vector<int32_t> avail((size_t)n);
  for (int i = 0; i < n; i++) avail[i] = i;
  for (int h = 0; h < H; h++) {
    const int32_t* d = draws + S * (size_t)h;
    int done = 0;
    for (; done < S; done++) {
      const int32_t r = d[done], size = n - done;
      if (r < 0 || r > size - 1) break;
      sets[S * (size_t)h + done] = avail[r];
      avail[r] = avail[size - 1];  // swap with the back; the pop is `size` one smaller in the next round
    }
    // the list of the next set is whole again: only the slots drawn from were written, and slot r of the whole list holds r
    for (int i = 0; i < done; i++) avail[d[i]] = d[i];
    if (done < S) return false;
  }
  return true;
}

}  // namespace orbfe
