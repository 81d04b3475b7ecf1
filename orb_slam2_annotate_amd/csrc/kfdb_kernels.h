// kfdb_kernels.h -- argument blocks and launchers of the key-frame database kernels (k_kfdb.hip; host side: kfdb.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbfe {

// The stored BowVectors as one CSR.  Slot s is the s-th key frame in list (insertion) order; an erased key frame
// keeps its slot with n = 0 until the host compacts the arrays.
struct KfdbSlot { uint32_t off, n; };

struct KfdbStore {
  const uint32_t* words;   // ascending inside a slot
  const double* values;
  const KfdbSlot* slots;
  int nSlots;
};

// Q queries as CSR (words ascending and unique per query) and the per-(query, slot) workspace, stride nSlots.
struct KfdbQueries {
  const int32_t* qOff;     // [Q + 1]
  const uint32_t* qWords;
  const double* qValues;
  int maxWords;            // longest query: sizes the LDS copy
  const int32_t* exclOff;  // [Q + 1] or NULL
  const uint32_t* exclSlots;
  int nExcl;               // exclOff[Q]
  uint32_t* common;        // [Q * nSlots] shared words
  uint32_t* minWord;       // [Q * nSlots] smallest shared word (only read where common > 0)
  uint32_t* surv;          // [Q * nSlots] survivors of the word-count filter, in slot order
  int32_t* nSurv;          // [Q]
  // results, `capacity` per query, in the order of the reference's lKFsSharingWords
  int capacity;
  uint32_t* outSlot; int32_t* outCommon; float* outScore;
};

constexpr int kKfdbLdsWords = 12288;  // queries up to this many words are searched in LDS (48 KB), longer ones in global memory

void launch_kfdb_query(hipStream_t s, const KfdbStore& st, const KfdbQueries& q, int nQueries);
// L1Scoring::score of one query (query 0 of q) against nIds named slots
void launch_kfdb_score(hipStream_t s, const KfdbStore& st, const KfdbQueries& q, const uint32_t* slotIds, int nIds, double* scores);

}  // namespace orbfe
