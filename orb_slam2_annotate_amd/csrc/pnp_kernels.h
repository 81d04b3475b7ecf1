// pnp_kernels.h -- argument blocks and launchers of the two PnPsolver kernels (k_pnp.hip; host side: pnp.hip).  The
// arithmetic is pnp_math.h.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pnp_math.h"

namespace orbfe {

constexpr int kPnpThreads = 256;  // k_pnp_ransac: four waves, one wave per hypothesis; k_pnp_refine: one record
constexpr int kPnpWavesPerBlock = kPnpThreads / 64;

// the point arrays and outputs both kernels share.  nItems = hypotheses (k_pnp_ransac) or Refine records (k_pnp_refine)
struct PnpArgs {
  int nItems;
  const PnpCandidate* cands;
  const int32_t* itemCand;  // [nItems] candidate of the item
  const float* p3d;         // [N * 3]
  const float* p2d;         // [N * 2]
  const float* maxErr2;     // [N]
  const int32_t* sets;      // k_pnp_ransac: [nItems * 4] indices local to the candidate
  const int32_t* idxOff;    // k_pnp_refine: [nItems + 1] where the record's index list begins in idx
  const int32_t* idx;       // k_pnp_refine: the set bits of the record's mask, ascending, local to the candidate
  int32_t* nInliers;        // [nItems]
  float* pose;              // [nItems * 12] R row-major, t
  uint32_t* words;          // [sum over candidates of items_k * words_k]
  uint8_t* status;          // [nItems]
};

void launch_pnp_ransac(hipStream_t s, const PnpArgs& a);
void launch_pnp_refine(hipStream_t s, const PnpArgs& a);

}  // namespace orbfe
