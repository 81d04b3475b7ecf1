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

}  // namespace orbfe
