// mappoints_host.h -- the host side of the device map-point table (mappoints.hip: orbfe_mappoints_*) that needs no device:
// argument checks, the table's slab layout and the interleaving of an update's records.  Plain C++ without a HIP
// include, so tests/cpp/mappoints_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "../../include/orbfe.h"

namespace orbfe {

constexpr int kMapPointsMaxCapacity = 1 << 24;

inline size_t mp_align(size_t bytes) { return (bytes + 255) & ~(size_t)255; }

// the table's slab: two 16-byte records per slot -- (X, Y, Z, min_dist) and (nx, ny, nz, max_dist) --, the 32-byte
// descriptors, one flag byte per slot
struct MapPointsLayout { size_t oRec, oDesc, oFlags, total; };
inline MapPointsLayout mappoints_layout(int capacity) {
  const size_t c = (size_t)(capacity > 0 ? capacity : 1);
  MapPointsLayout L;
  L.oRec = 0;
  L.oDesc = mp_align(c * 32);
  L.oFlags = L.oDesc + mp_align(c * 32);
  L.total = L.oFlags + mp_align(c);
  return L;
}

inline const char* mappoints_check_create(int capacity, const void* out) {
  if (!out) return "NULL argument";
  if (capacity <= 0 || capacity > kMapPointsMaxCapacity) return "capacity must be 1 .. 16777216";
  return nullptr;
}

// a slot list of a table of `capacity` slots; NULL when it is fine, else what is wrong with it
inline const char* mappoints_check_slots(int capacity, int n, const int32_t* slot) {
  if (n < 0) return "negative count";
  if (n > 0 && !slot) return "NULL slot list";
  for (int i = 0; i < n; i++)
    if (slot[i] < 0 || slot[i] >= capacity) return "slot outside [0, capacity)";
  return nullptr;
}

inline const char* mappoints_check_update(int capacity, int n, const int32_t* slot, const float* pos, const float* normal,
                                          const float* min_dist, const float* max_dist, const uint8_t* flags) {
  if (const char* e = mappoints_check_slots(capacity, n, slot)) return e;
  if (n > 0 && (!pos || !normal || !min_dist || !max_dist || !flags)) return "NULL array";
  return nullptr;
}

// the two 16-byte records of each of the n points of an update, as the scatter kernel reads them: rec[8 i ..] =
// (X, Y, Z, min_dist, nx, ny, nz, max_dist), 8 n floats
inline void mappoints_pack_records(float* rec, int n, const float* pos, const float* normal, const float* min_dist,
                                   const float* max_dist) {
  for (int i = 0; i < n; i++) {
    float* r = rec + (size_t)i * 8;
    r[0] = pos[3 * i]; r[1] = pos[3 * i + 1]; r[2] = pos[3 * i + 2]; r[3] = min_dist[i];
    r[4] = normal[3 * i]; r[5] = normal[3 * i + 1]; r[6] = normal[3 * i + 2]; r[7] = max_dist[i];
  }
}


// The operands of orbfe_project_fuse / orbfe_fuse_mappoints that need neither handle: the slot list of a table of `capacity`
// slots, K poses (at most kFuseMaxPoses, the kernel's LDS holds them) and -- with_graph -- the K kf slots of a graph of
// kf_capacity key frames.  n_levels > 0: the caller's level tables hold that many entries, and no pose may predict past them.
constexpr int kFuseMaxPoses = 64, kFuseMaxPoseLevels = 64;
inline const char* fuse_check_operands(int capacity, int n, const int32_t* slot, int K, const int32_t* kf_slot, bool with_graph,
                                       int kf_capacity, const orbfe_camera_pose* pose, int n_levels) {
  if (K < 0) return "negative number of key frames";
  if (K > kFuseMaxPoses) return "more than 64 key frames in one call";
  if (const char* e = mappoints_check_slots(capacity, n, slot)) return e;
  if (K > 0 && !pose) return "NULL pose array";
  if (K > 0 && with_graph && !kf_slot) return "NULL kf_slot array";
  for (int k = 0; k < K; k++) {
    if (pose[k].n_levels < 1 || pose[k].n_levels > kFuseMaxPoseLevels) return "bad pose (n_levels must be 1 .. 64)";
    if (n_levels > 0 && pose[k].n_levels > n_levels) return "a pose predicts more levels than the level tables hold";
    if (with_graph && (kf_slot[k] < 0 || kf_slot[k] >= kf_capacity)) return "kf slot outside [0, kf_capacity)";
  }
  return nullptr;
}

// The operands of orbfe_project_last_frame / orbfe_search_last_frame_mappoints (K = 1, offsets = {0, n}, with_octave) and of
// orbfe_project_keyframe / orbfe_search_keyframe_mappoints_multi that need no handle: K jobs (at most kTrackMaxJobPoses) over
// concatenated lists -- offsets[K + 1] starts at 0 and never descends --, the slots of a table of `capacity` slots, one pose per
// job and -- with_octave -- the last frame's octaves.  n_levels > 0: the caller's level table holds that many entries; no
// octave and no pose may point past it.  Nothing is read past what K and offsets[K] say.
constexpr int kTrackMaxJobPoses = 64;
inline const char* track_check_operands(int capacity, int K, const int32_t* offsets, const int32_t* slot, bool with_octave,
                                        const int32_t* last_octave, const orbfe_camera_pose* pose, int n_levels) {
  if (K < 0) return "negative number of jobs";
  if (K > kTrackMaxJobPoses) return "more than 64 jobs in one call";
  if (K == 0) return nullptr;
  if (!offsets) return "NULL offsets";
  if (offsets[0] != 0) return "offsets must start at 0";
  for (int k = 0; k < K; k++)
    if (offsets[k + 1] < offsets[k]) return offsets[k + 1] < 0 ? "negative count" : "offsets descend";
  const int total = offsets[K];
  if (const char* e = mappoints_check_slots(capacity, total, slot)) return e;
  if (!pose) return "NULL pose array";
  for (int k = 0; k < K; k++) {
    if (pose[k].n_levels < 1 || pose[k].n_levels > kFuseMaxPoseLevels) return "bad pose (n_levels must be 1 .. 64)";
    if (n_levels > 0 && pose[k].n_levels > n_levels) return "a pose predicts more levels than the level table holds";
  }
  if (with_octave) {
    if (total > 0 && !last_octave) return "NULL octave array";
    for (int i = 0; i < total; i++)
      if (last_octave[i] < 0 || (n_levels > 0 && last_octave[i] >= n_levels)) return "octave outside the level table";
  }
  return nullptr;
}

// The operands of orbfe_project_sim3 that need no handle: n_legs legs (at most kSim3MaxLegRecords) over concatenated lists --
// offsets[n_legs + 1] starts at 0 and never descends --, slots of a table of `capacity` slots or -1 (no map point), one leg
// record each.  n_levels > 0: the caller's level tables hold that many entries and no leg may predict past them.  Nothing is
// read past what n_legs and offsets[n_legs] say.
constexpr int kSim3MaxCandidates = 64, kSim3MaxLegRecords = 2 * kSim3MaxCandidates;
inline const char* sim3_check_slots(int capacity, int n, const int32_t* slot) {
  if (n < 0) return "negative count";
  if (n > 0 && !slot) return "NULL slot list";
  for (int i = 0; i < n; i++)
    if (slot[i] < -1 || slot[i] >= capacity) return "slot outside [-1, capacity)";
  return nullptr;
}
inline const char* sim3_check_offsets(int K, const int32_t* offsets) {
  if (!offsets) return "NULL offsets";
  if (offsets[0] != 0) return "offsets must start at 0";
  for (int k = 0; k < K; k++)
    if (offsets[k + 1] < offsets[k]) return offsets[k + 1] < 0 ? "negative count" : "offsets descend";
  return nullptr;
}
inline const char* sim3_check_leg_records(int n, const orbfe_sim3_leg* legs, int n_levels) {
  if (n > 0 && !legs) return "NULL leg array";
  for (int l = 0; l < n; l++) {
    if (legs[l].n_levels < 1 || legs[l].n_levels > kFuseMaxPoseLevels) return "bad leg (n_levels must be 1 .. 64)";
    if (n_levels > 0 && legs[l].n_levels > n_levels) return "a leg predicts more levels than the level table holds";
  }
  return nullptr;
}
inline const char* sim3_check_legs(int capacity, int n_legs, const int32_t* offsets, const int32_t* slot, const orbfe_sim3_leg* legs,
                                   int n_levels) {
  if (n_legs < 0) return "negative number of legs";
  if (n_legs > kSim3MaxLegRecords) return "more than 128 legs in one call";
  if (n_legs == 0) return nullptr;
  if (const char* e = sim3_check_offsets(n_legs, offsets)) return e;
  if (const char* e = sim3_check_slots(capacity, offsets[n_legs], slot)) return e;
  return sim3_check_leg_records(n_legs, legs, n_levels);
}

// The operands of orbfe_search_by_sim3_mappoints_multi that need no handle and no view: KF1's n1 slots, K candidates (at most
// kSim3MaxCandidates) over the concatenated slot2[] (offsets2[K + 1]), the two leg arrays, the matched slots ([K * n1], NULL:
// none; -1 or a slot of the table) and -- with_graph -- the K kf slots of a graph of kf_capacity key frames.
inline const char* sim3_check_search(int capacity, int n1, const int32_t* slot1, int K, const int32_t* offsets2, const int32_t* slot2,
                                     const orbfe_sim3_leg* legs12, const orbfe_sim3_leg* legs21, const int32_t* matched12_in,
                                     const int32_t* kf2_slot, bool with_graph, int kf_capacity, int n_levels) {
  if (K < 0) return "negative number of candidates";
  if (K > kSim3MaxCandidates) return "more than 64 candidates in one call";
  if (n_levels < 1 || n_levels > kFuseMaxPoseLevels) return "n_levels must be 1 .. 64";
  if (const char* e = sim3_check_slots(capacity, n1, slot1)) return e;
  if (K == 0) return nullptr;
  if (const char* e = sim3_check_offsets(K, offsets2)) return e;
  if (const char* e = sim3_check_slots(capacity, offsets2[K], slot2)) return e;
  if (const char* e = sim3_check_leg_records(K, legs12, n_levels)) return e;
  if (const char* e = sim3_check_leg_records(K, legs21, n_levels)) return e;
  if (matched12_in)
    for (size_t i = 0; i < (size_t)K * (size_t)n1; i++)
      if (matched12_in[i] < -1 || matched12_in[i] >= capacity) return "matched slot outside [-1, capacity)";
  if (with_graph) {
    if (!kf2_slot) return "NULL kf2_slot array";
    for (int k = 0; k < K; k++)
      if (kf2_slot[k] < 0 || kf2_slot[k] >= kf_capacity) return "kf slot outside [0, kf_capacity)";
  }
  return nullptr;
}

}  // namespace orbfe
