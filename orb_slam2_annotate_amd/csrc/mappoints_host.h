// mappoints_host.h -- the host side of the device map-point table (mappoints.hip: orbfe_mappoints_*) that needs no device:
// argument checks, the table's slab layout and the packing of an update into the staging buffer.  Plain C++ without a HIP
// include, so tests/cpp/mappoints_host_san.cpp runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cstring>

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

// one update in the staging buffer, in the order the scatter kernel reads it: slots | records | flags | descriptors
struct MapPointsStage { size_t oSlot, oRec, oFlags, oDesc, total; };
inline MapPointsStage mappoints_stage_layout(int n, bool withDesc) {
  const size_t c = (size_t)(n > 0 ? n : 1);
  MapPointsStage S;
  S.oSlot = 0;
  S.oRec = mp_align(c * 4);
  S.oFlags = S.oRec + mp_align(c * 32);
  S.oDesc = S.oFlags + mp_align(c);
  S.total = S.oDesc + (withDesc ? mp_align(c * 32) : 0);
  return S;
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

// h: S.total bytes
inline void mappoints_pack(uint8_t* h, const MapPointsStage& S, int n, const int32_t* slot, const float* pos, const float* normal,
                           const float* min_dist, const float* max_dist, const uint8_t* desc, const uint8_t* flags) {
  if (n <= 0) return;
  std::memcpy(h + S.oSlot, slot, (size_t)n * 4);
  float* rec = reinterpret_cast<float*>(h + S.oRec);
  for (int i = 0; i < n; i++) {
    float* r = rec + (size_t)i * 8;
    r[0] = pos[3 * i]; r[1] = pos[3 * i + 1]; r[2] = pos[3 * i + 2]; r[3] = min_dist[i];
    r[4] = normal[3 * i]; r[5] = normal[3 * i + 1]; r[6] = normal[3 * i + 2]; r[7] = max_dist[i];
  }
  std::memcpy(h + S.oFlags, flags, (size_t)n);
  if (desc) std::memcpy(h + S.oDesc, desc, (size_t)n * 32);
}

}  // namespace orbfe
