// loopcorrect_kernels.h -- launch interface of k_loopcorrect.hip (host side: loopcorrect.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "match_kernels.h"
#include "obsgraph_kernels.h"

namespace orbfe {

// the unit of the claim's grid: 256 consecutive positions p = k * width + idx, as four wave-sized chunks with one keep
// mask each (positions are global: a chunk or a block may span rows)
constexpr int kLcBlockEntries = 256, kLcChunksPerBlock = kLcBlockEntries / 64;

// One orbfe_correct_loop_mappoints call.  kfSlot / firstOf [K] (firstOf[k]: the lowest k' with kfSlot[k'] == kfSlot[k]),
// corrected / noncorrected [K][8], owCorrected [K][3], skip [nSkip].  rank: the graph's kf_capacity int32, -1 everywhere
// between calls.  Workspaces, none of which needs clearing: first [point_capacity], keepMask [nBlocks][4], blockCount
// [nBlocks] (each block's exclusive prefix afterwards).  slotOut / refOut / validOut hold `count` entries.
struct LoopCorrectArgs {
  int K, nBlocks, nSkip, nLevels;
  const int32_t *kfSlot, *firstOf, *skip;
  const double *corrected, *noncorrected;
  const float *owCorrected, *scale;
  int32_t *rank, *first;
  unsigned long long* keepMask;
  int32_t *blockCount, *count;
  int32_t *slotOut, *refOut;
  uint8_t* validOut;
};

// rank[kfSlot[k]] = k for every first occurrence; then mark, skip, min, keep, scan: *count and the keep masks stand
void launch_lc_claim(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, const LoopCorrectArgs& a);
// the lists, the positions, normal and range of the `count` claimed points (count: what launch_lc_claim left in *count,
// read back by the host), and the K key frames' Ow
void launch_lc_apply(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, const MapPointsDevice& table, const LoopCorrectArgs& a,
                     int count);
// rank[kfSlot[k]] = -1: the table idle again
void launch_lc_release(hipStream_t s, const LoopCorrectArgs& a);

// One orbfe_gba_update_mappoints call: slot / inGba [n], posGba [n][3]; kfSlot / reached [m], TcwBef / TwcNew [m][16]; index:
// the graph's rank table (as above); moved [n]
struct GbaUpdateArgs {
  int n, m;
  const int32_t* slot;
  const uint8_t* inGba;
  const float* posGba;
  const int32_t* kfSlot;
  const uint8_t* reached;
  const float *TcwBef, *TwcNew;
  int32_t* index;
  uint8_t* moved;
};
void launch_gba_update(hipStream_t s, const ObsGraphDevice& g, const MapPointsDevice& table, const GbaUpdateArgs& a);

}  // namespace orbfe
