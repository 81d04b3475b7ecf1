// obsgraph_kernels.h -- launch interface of k_obsgraph.hip (host side: obsgraph.hip).  The table's records are
// obsgraph_host.h's: the kernels read what the host mirror wrote, nothing else.
#pragma once
#include <hip/hip_runtime.h>

#include "match_kernels.h"
#include "obsgraph_host.h"

namespace orbfe {

// the vote counters of a query live in LDS up to this many kf slots (32 KiB of the workgroup's LDS), above it in a
// workspace slice of kf_capacity int32 per query
constexpr int kObsVotesLdsKeyFrames = 8192;

struct ObsGraphDevice {
  ObsEntry* rows;      // [point_capacity][row_width]
  ObsPointMeta* meta;  // [point_capacity]
  ObsKeyFrame* kf;     // [kf_capacity]
  int rowWidth, pointCap, kfCap;
};

// rewrites n rows (and their meta records) from a staged block: slot[n], meta[n], rowOf[n] (index of the row's
// row_width entries in `rows`, -1: the row is empty and only its meta record is written)
void launch_obs_scatter(hipStream_t s, const ObsGraphDevice& g, int n, const int32_t* slot, const ObsPointMeta* meta,
                        const int32_t* rowOf, const ObsEntry* rows);

// query q = qSlots [qOff[q], qOff[q+1]); out*: [nQueries][capacity]; counters: nQueries * kf_capacity int32 when
// kf_capacity > kObsVotesLdsKeyFrames (else unused)
void launch_obs_votes(hipStream_t s, const ObsGraphDevice& g, int nQueries, const int32_t* qOff, const int32_t* qSlots,
                      const int32_t* self, int capacity, int32_t* outKf, int32_t* outWeight, int32_t* count, int32_t* counters);

// feature f: point slot[f] seen at octave[f] by candidate cand[f] (an index into kfSlot / nMps / nRedundant, which the
// caller has zeroed)
void launch_obs_culling(hipStream_t s, const ObsGraphDevice& g, int nFeatures, const int32_t* cand, const int32_t* kfSlot,
                        const int32_t* slot, const uint8_t* octave, int32_t* nMps, int32_t* nRedundant);

// pos != NULL: positions from pos[n*3], results to normal[n*3] / minDist / maxDist; pos == NULL: positions from, results
// into `table`.  valid[n] either way.
void launch_obs_normal_depth(hipStream_t s, const ObsGraphDevice& g, int n, const int32_t* slot, const float* pos,
                             const float* scale, int nLevels, float* normal, float* minDist, float* maxDist, uint8_t* valid,
                             const MapPointsDevice* table);

// ---- k_kfpoints.hip: KeyFrame::mvpMapPoints, the rows of point slots per kf slot ----

// the unit of the union's grid: 1024 consecutive positions p = k * width + idx of one query (k: the key frame's place in
// the query), as 16 wave-sized chunks.  width is a multiple of 64, so a chunk never spans two rows.
constexpr int kKfBlockEntries = 1024, kKfChunksPerBlock = kKfBlockEntries / 64;

struct KfPointsDevice {
  int32_t* rows;  // [kf_capacity][width], -1: NULL; entries at and past len[kf] are never read
  int32_t* len;   // [kf_capacity]: N of the key frame
  int width;
};

// rewrites n rows from a staged block: kf[n], len[n], rowOf[n] (index of the row's `width` entries in `rows`, -1: the
// row is empty and only its length is written)
void launch_kf_scatter(hipStream_t s, const KfPointsDevice& t, int n, const int32_t* kf, const int32_t* len, const int32_t* rowOf,
                       const int32_t* rows);

// One group of queries of orbfe_obsgraph_keyframe_points_union.  Query q: the kf slots qKf [qOff[q], qOff[q+1]); its
// blocks are blkOff[q] .. blkOff[q+1] of a flat grid of nBlocks = blkOff[nQueries].  Workspaces, none of which needs
// clearing: first [nQueries][point_capacity], keepMask [nBlocks][16], blockCount [nBlocks] (holds each block's exclusive
// prefix within its query afterwards).  out [nQueries][capacity], count [nQueries].  Five launches on s.
struct KfUnionArgs {
  int nQueries, nBlocks, capacity;
  const int32_t *qOff, *qKf, *blkOff;
  int32_t* first;
  unsigned long long* keepMask;
  int32_t *blockCount, *out, *count;
};
void launch_kf_union(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, const KfUnionArgs& a);

// KeyFrame::TrackedMapPoints for kf[n] in one launch, a wave per key frame
void launch_kf_tracked(hipStream_t s, const ObsGraphDevice& g, const KfPointsDevice& t, int n, const int32_t* kf, int minObs,
                       int32_t* count);

// ---- k_obsdesc.hip: KeyFrame::mDescriptors per kf slot and MapPoint::ComputeDistinctiveDescriptors over the rows ----

struct KfDescDevice {
  const uint8_t* desc;  // [kf_capacity][width][32]; rows at and past a key frame's count are never read.  NULL: nothing set yet
  int width;
};

// a row whose entry count is above this runs in the form whose lanes hold four descriptors each
constexpr int kObsDescOneChunk = 64;

// MapPoint::ComputeDistinctiveDescriptors for slot[n], a wave per point.  valid[n]; where valid: bestKf / bestIdx [n] and
// the winner's 32 bytes -- into outDesc[n][32] (table == NULL) or into the table's descriptor of the slot.  maxCount: the
// largest entry count among the listed rows (from the mirror); above kObsDescOneChunk a second launch takes the long rows.
void launch_obs_distinctive(hipStream_t s, const ObsGraphDevice& g, const KfDescDevice& kd, int n, const int32_t* slot, int maxCount,
                            int32_t* bestKf, int32_t* bestIdx, uint8_t* outDesc, uint8_t* valid, const MapPointsDevice* table);

}  // namespace orbfe
