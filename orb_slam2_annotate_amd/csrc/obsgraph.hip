// obsgraph.hip -- host side of the device observation graph (include/orbfe.h: orbfe_obsgraph; kernels: k_obsgraph.hip).
// Reference: MapPoint::mObservations and the four loops over it -- KeyFrame::UpdateConnections (src/KeyFrame.cc:311-403),
// Tracking::UpdateLocalKeyFrames (src/Tracking.cc:1339-1455), LocalMapping::KeyFrameCulling (src/LocalMapping.cc:710-774),
// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:360-404).
//
// The table lives in one slab of the pool: rows [point_capacity][row_width] of 8-byte entries, one 16-byte record per
// point slot, one 24-byte record per kf slot.  The host mirror (obsgraph_host.h) is the truth: a mutation changes the
// mirror alone, so it needs no device, and marks what it touched; every call that reads the table on the device first
// rewrites the marked rows, each as a whole, through one staged copy and one scatter launch.  Every operand is checked on
// the host BEFORE anything is enqueued, the kernels read only what the host wrote, and everything runs on the handle's one
// stream and is complete on return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "host_internal.h"
#include "match_kernels.h"
#include "obsgraph_handle.h"
#include "obsgraph_host.h"
#include "obsgraph_kernels.h"

using namespace orbfe;

static_assert(sizeof(orbfe_observation) == sizeof(ObsEntry), "orbfe_observation is the table's entry");

namespace {

// the marked rows and key frames onto the device; the marks are dropped only when everything has arrived
int obs_flush(orbfe_obsgraph* g) {
  ObsGraphMirror& h = g->h;
  Arena* ar = &g->arena;
  const size_t rw = (size_t)h.rowWidth;
  if (h.kfDirtyHi > h.kfDirtyLo)
    HIPCHK(hipMemcpyAsync(g->d.kf + h.kfDirtyLo, h.kfs.data() + h.kfDirtyLo, (size_t)(h.kfDirtyHi - h.kfDirtyLo) * sizeof(ObsKeyFrame),
                          hipMemcpyHostToDevice, ar->stream));
  const size_t perRow = 4 + sizeof(ObsPointMeta) + 4 + rw * sizeof(ObsEntry);
  const size_t rowsPerChunk = std::max<size_t>(1, kObsFlushChunkBytes / perRow);
  for (size_t at = 0; at < h.dirtyRows.size(); at += rowsPerChunk) {
    const size_t n = std::min(rowsPerChunk, h.dirtyRows.size() - at);
    const int32_t* marked = h.dirtyRows.data() + at;
    size_t nRows = 0;
    for (size_t i = 0; i < n; i++) nRows += !h.rows[(size_t)marked[i]].empty();
    int32_t *dSlot, *dRowOf;
    ObsPointMeta* dMeta;
    ObsEntry* dRows;
    auto stage = [&](Arena* a) -> hipError_t {
      TRY(up(a, &dSlot, marked, n));
      TRY(up_pack(a, &dMeta, n, [&](ObsPointMeta* m) {
        for (size_t i = 0; i < n; i++) m[i] = h.meta[(size_t)marked[i]];
      }));
      TRY(up_pack(a, &dRowOf, n, [&](int32_t* rowOf) {
        int32_t r = 0;
        for (size_t i = 0; i < n; i++) rowOf[i] = h.rows[(size_t)marked[i]].empty() ? -1 : r++;
      }));
      return up_pack(a, &dRows, nRows * rw, [&](ObsEntry* rows) {  // the rows that hold something, each padded with zeros
        for (size_t i = 0; i < n; i++) {
          const std::vector<ObsEntry>& row = h.rows[(size_t)marked[i]];
          if (row.empty()) continue;
          std::memset(rows, 0, rw * sizeof(ObsEntry));
          std::memcpy(rows, row.data(), row.size() * sizeof(ObsEntry));
          rows += rw;
        }
      });
    };
    HIPCHK(arena_stage(ar, g->device, stage));
    HIPCHK(flush(ar));
    launch_obs_scatter(ar->stream, g->d, (int)n, dSlot, dMeta, dRowOf, dRows);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ar->stream));  // the arena is begun anew by the next chunk
  }
  HIPCHK(hipStreamSynchronize(ar->stream));
  h.flushed();
  return ORBFE_OK;
}

}  // namespace

int orbfe::obs_invalid(const char* fn, const char* what) { return fail(ORBFE_ERR_INVALID, std::string(fn) + ": " + what); }

// what every call that reads the table on the device starts with (the handle locked)
int orbfe::obs_ready(orbfe_obsgraph* g) {
  HIPCHK(arena_stream(&g->arena, g->device));
  ObsGraphMirror& h = g->h;
  if (!g->table.p) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };  // each of the slab's three arrays starts a line
    const size_t oMeta = al((size_t)h.pointCap * h.rowWidth * sizeof(ObsEntry)), oKf = oMeta + al((size_t)h.pointCap * sizeof(ObsPointMeta)),
                 total = oKf + al((size_t)h.kfCap * sizeof(ObsKeyFrame));
    Slab s;
    HIPCHK(slab_get(g->device, total, &s));
    uint8_t* b = static_cast<uint8_t*>(s.p);
    // every record from the mirror; of the rows, the ones that hold something
    hipError_t e = hipMemcpyAsync(b + oMeta, h.meta.data(), (size_t)h.pointCap * sizeof(ObsPointMeta), hipMemcpyHostToDevice, g->arena.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->arena.stream);
    if (e != hipSuccess) { slab_put(&s); HIPCHK(e); }
    g->table = s;
    g->d.rows = reinterpret_cast<ObsEntry*>(b); g->d.meta = reinterpret_cast<ObsPointMeta*>(b + oMeta);
    g->d.kf = reinterpret_cast<ObsKeyFrame*>(b + oKf);
    g->d.rowWidth = h.rowWidth; g->d.pointCap = h.pointCap; g->d.kfCap = h.kfCap;
    h.flushed();
    h.kfDirtyLo = 0; h.kfDirtyHi = h.kfCap;
    for (int i = 0; i < h.pointCap; i++)
      if (!h.rows[(size_t)i].empty()) h.touch(i);
  }
  if (h.dirtyRows.empty() && h.kfDirtyHi <= h.kfDirtyLo) return ORBFE_OK;
  return obs_flush(g);
}

// host_internal.h: the handle's serialisation for a scope, for a host file that reads the rows on the device
orbfe::ObsGraphLock::ObsGraphLock(orbfe_obsgraph* g) {
  if (!g) return;
  g->m.lock();
  held = g;
  device = g->device; pointCap = g->h.pointCap; kfCap = g->h.kfCap;
}
orbfe::ObsGraphLock::~ObsGraphLock() {
  if (held) held->m.unlock();
}
int orbfe::ObsGraphLock::table_ready() {
  if (!held) return ORBFE_OK;
  if (int rc = obs_ready(held)) return rc;
  graph = &held->d;
  return ORBFE_OK;
}

namespace {

int invalid(const char* fn, const char* what) { return obs_invalid(fn, what); }

// pos == NULL: the table form (positions from and results into *table)
int normal_depth_run(orbfe_obsgraph* g, int n, const int32_t* slot, const float* pos, const float* scale, int n_levels, float* normal,
                     float* min_dist, float* max_dist, uint8_t* valid, const MapPointsDevice* table) {
  const size_t q = (size_t)n;
  Arena* ar = &g->arena;
  int32_t* dSlot;
  float *dScale, *dPos = nullptr, *dNormal = nullptr, *dMin = nullptr, *dMax = nullptr;
  uint8_t* dValid;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dSlot, slot, q));
    TRY(up(a, &dScale, scale, (size_t)n_levels));
    if (pos) TRY(up(a, &dPos, pos, 3 * q));
    open_span(a);
    dValid = carve<uint8_t>(a, q);
    if (!table) {
      dMin = carve<float>(a, q);
      dMax = carve<float>(a, q);
      dNormal = carve<float>(a, 3 * q);
    }
    return close_span(a);
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  HIPCHK(flush(ar));
  launch_obs_normal_depth(ar->stream, g->d, n, dSlot, dPos, dScale, n_levels, dNormal, dMin, dMax, dValid, table);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const uint8_t* v = mirror_of(ar, dValid);
  if (valid) std::memcpy(valid, v, q);
  if (!table) {
    const float *hn = mirror_of(ar, dNormal), *lo = mirror_of(ar, dMin), *hi = mirror_of(ar, dMax);
    for (size_t i = 0; i < q; i++) {  // valid = 0 writes nothing
      if (!v[i]) continue;
      normal[3 * i] = hn[3 * i]; normal[3 * i + 1] = hn[3 * i + 1]; normal[3 * i + 2] = hn[3 * i + 2];
      min_dist[i] = lo[i];
      max_dist[i] = hi[i];
    }
  }
  return ORBFE_OK;
}

const char* check_scale(const float* scale, int n_levels) {
  if (n_levels < 1 || n_levels > 256) return "n_levels must be 1 .. 256";
  if (!scale) return "NULL scale_factors";
  return nullptr;
}

}  // namespace

extern "C" int orbfe_obsgraph_create(int device, int point_capacity, int kf_capacity, int row_width, orbfe_obsgraph** out) {
  if (const char* e = obsgraph_check_create(device, point_capacity, kf_capacity, row_width, out)) return invalid("obsgraph_create", e);
  *out = nullptr;
  orbfe_obsgraph* g = new (std::nothrow) orbfe_obsgraph();
  if (!g) return fail(ORBFE_ERR_NOMEM, "out of memory");
  g->device = device;
  try {
    g->h.init(point_capacity, kf_capacity, row_width);
  } catch (const std::bad_alloc&) {
    delete g;
    return fail(ORBFE_ERR_NOMEM, "out of memory");
  }
  *out = g;  // the device is first touched by the first call that reads the table there
  return ORBFE_OK;
}

extern "C" void orbfe_obsgraph_destroy(orbfe_obsgraph* g) {
  if (!g) return;
  if (g->arena.stream) {
    (void)hipSetDevice(g->device);
    (void)hipStreamSynchronize(g->arena.stream);
    slab_put(&g->table);
    slab_put(&g->kfTable);
    slab_put(&g->descTable);
  }
  delete g;  // (the arena's end: the stream, then the buffers)
}

extern "C" int orbfe_obsgraph_clear(orbfe_obsgraph* g) {
  if (!g) return invalid("obsgraph_clear", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  g->h.clear();  // the slab stays with the handle
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_set_keyframes(orbfe_obsgraph* g, int n, const int32_t* kf_slot, const int64_t* kf_id, const float* Ow,
                                            const uint8_t* bad) {
  if (!g) return invalid("obsgraph_set_keyframes", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.set_keyframes(n, kf_slot, kf_id, Ow, bad)) return invalid("obsgraph_set_keyframes", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_set_points(orbfe_obsgraph* g, int n, const int32_t* slot, const uint8_t* bad, const int32_t* ref_kf_slot) {
  if (!g) return invalid("obsgraph_set_points", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.set_points(n, slot, bad, ref_kf_slot)) return invalid("obsgraph_set_points", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_add_observations(orbfe_obsgraph* g, int n, const int32_t* slot, const int32_t* kf_slot, const uint16_t* idx,
                                               const uint8_t* octave, const uint8_t* stereo) {
  if (!g) return invalid("obsgraph_add_observations", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  bool full;
  if (const char* e = g->h.add_observations(n, slot, kf_slot, idx, octave, stereo, &full))
    return full ? fail(ORBFE_ERR_CAPACITY, std::string("obsgraph_add_observations: ") + e) : invalid("obsgraph_add_observations", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_erase_observations(orbfe_obsgraph* g, int n, const int32_t* slot, const int32_t* kf_slot, uint8_t* became_bad) {
  if (!g) return invalid("obsgraph_erase_observations", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.erase_observations(n, slot, kf_slot, became_bad)) return invalid("obsgraph_erase_observations", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_erase_keyframe(orbfe_obsgraph* g, int kf_slot, int32_t* out_slots, int capacity, int* n_out) {
  if (!g) return invalid("obsgraph_erase_keyframe", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  bool over;
  if (const char* e = g->h.erase_keyframe(kf_slot, out_slots, capacity, n_out, &over))
    return over ? fail(ORBFE_ERR_CAPACITY, std::string("obsgraph_erase_keyframe: ") + e) : invalid("obsgraph_erase_keyframe", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_get_row(orbfe_obsgraph* g, int from_device, int slot, orbfe_observation* entries, int32_t* n_entries,
                                      int32_t* n_obs, uint8_t* bad, int32_t* ref_kf_slot) {
  if (!g || !entries || !n_entries || !n_obs || !bad || !ref_kf_slot) return invalid("obsgraph_get_row", "NULL argument");
  if (slot < 0 || slot >= g->h.pointCap) return invalid("obsgraph_get_row", "slot outside [0, point_capacity)");
  std::lock_guard<std::mutex> lk(g->m);
  const size_t rw = (size_t)g->h.rowWidth;
  ObsPointMeta m;
  std::memset(entries, 0, rw * sizeof(orbfe_observation));
  if (!from_device) {
    m = g->h.meta[(size_t)slot];
    const std::vector<ObsEntry>& r = g->h.rows[(size_t)slot];
    if (!r.empty()) std::memcpy(entries, r.data(), r.size() * sizeof(ObsEntry));
  } else {
    if (int rc = obs_ready(g)) return rc;
    Arena* ar = &g->arena;
    ObsPointMeta* hMeta;
    ObsEntry* hRow;
    auto stage = [&](Arena* a) { open_span(a); hMeta = carve<ObsPointMeta>(a, 1); hRow = carve<ObsEntry>(a, rw); return close_span(a); };
    HIPCHK(arena_stage(ar, g->device, stage));
    HIPCHK(fetch(ar, hMeta, g->d.meta + slot, 1));
    HIPCHK(fetch(ar, hRow, g->d.rows + (size_t)slot * rw, rw));
    HIPCHK(hipStreamSynchronize(ar->stream));
    m = *mirror_of(ar, hMeta);
    const int live = std::min(std::max(m.count, 0), (int)rw);
    if (live) std::memcpy(entries, mirror_of(ar, hRow), (size_t)live * sizeof(ObsEntry));
  }
  *n_entries = m.count; *n_obs = m.nObs; *bad = (uint8_t)m.bad; *ref_kf_slot = m.ref;
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_votes(orbfe_obsgraph* g, int n_queries, const int32_t* q_offsets, const int32_t* q_slots,
                                    const int32_t* self_kf_slot, int capacity, int32_t* kf_slot_out, int32_t* weight_out, int32_t* count) {
  const char* fn = "obsgraph_votes";
  if (!g || n_queries < 0 || capacity < 0) return invalid(fn, "bad argument");
  if (n_queries == 0) return ORBFE_OK;
  if (n_queries > 65535) return invalid(fn, "at most 65535 queries per call");
  if (!q_offsets || !self_kf_slot || !count || (capacity > 0 && (!kf_slot_out || !weight_out))) return invalid(fn, "NULL argument");
  const int Q = n_queries;
  if (q_offsets[0] != 0) return invalid(fn, "q_offsets[0] must be 0");
  for (int q = 0; q < Q; q++) {
    if (q_offsets[q + 1] < q_offsets[q]) return invalid(fn, "q_offsets must not descend");
    if (self_kf_slot[q] < -1 || self_kf_slot[q] >= g->h.kfCap) return invalid(fn, "self_kf_slot outside [-1, kf_capacity)");
  }
  const size_t nq = (size_t)q_offsets[Q];
  if (nq && !q_slots) return invalid(fn, "NULL q_slots");
  if (!g->h.slots_ok((int)nq, q_slots)) return invalid(fn, "slot outside [0, point_capacity)");
  std::lock_guard<std::mutex> lk(g->m);
  if (int rc = obs_ready(g)) return rc;
  const size_t cap = (size_t)capacity, nQ = (size_t)Q;
  Arena* ar = &g->arena;
  int32_t *dOff, *dSelf, *dSlots, *dCount, *dKf, *dW, *dCounters = nullptr;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dOff, q_offsets, nQ + 1));
    TRY(up(a, &dSelf, self_kf_slot, nQ));
    TRY(up(a, &dSlots, q_slots, nq));
    open_span(a);
    dCount = carve<int32_t>(a, nQ);
    dKf = carve<int32_t>(a, nQ * cap);
    dW = carve<int32_t>(a, nQ * cap);
    TRY(close_span(a));
    if (g->h.kfCap > kObsVotesLdsKeyFrames) dCounters = carve<int32_t>(a, nQ * (size_t)g->h.kfCap);
    return hipSuccess;
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  HIPCHK(flush(ar));
  launch_obs_votes(ar->stream, g->d, Q, dOff, dSlots, dSelf, capacity, dKf, dW, dCount, dCounters);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const int32_t *ns = mirror_of(ar, dCount), *hKf = mirror_of(ar, dKf), *hW = mirror_of(ar, dW);
  bool over = false;
  for (int q = 0; q < Q; q++) {
    count[q] = ns[q];
    const size_t m = std::min((size_t)std::max(ns[q], 0), cap);
    over |= (size_t)std::max(ns[q], 0) > cap;
    if (m) {
      std::memcpy(kf_slot_out + q * cap, hKf + q * cap, m * 4);
      std::memcpy(weight_out + q * cap, hW + q * cap, m * 4);
    }
  }
  if (over) return fail(ORBFE_ERR_CAPACITY, "obsgraph_votes: a query has more voted key frames than `capacity` (see count[])");
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_culling_counts(orbfe_obsgraph* g, int n_kf, const int32_t* kf_slot, const int32_t* offsets, const int32_t* slot,
                                             const uint8_t* octave, int32_t* n_mps, int32_t* n_redundant) {
  const char* fn = "obsgraph_culling_counts";
  if (!g || n_kf < 0) return invalid(fn, "bad argument");
  if (n_kf == 0) return ORBFE_OK;
  if (!kf_slot || !offsets || !n_mps || !n_redundant) return invalid(fn, "NULL argument");
  if (!g->h.kf_slots_ok(n_kf, kf_slot)) return invalid(fn, "kf slot outside [0, kf_capacity)");
  if (offsets[0] != 0) return invalid(fn, "offsets[0] must be 0");
  for (int c = 0; c < n_kf; c++)
    if (offsets[c + 1] < offsets[c]) return invalid(fn, "offsets must not descend");
  const size_t F = (size_t)offsets[n_kf], C = (size_t)n_kf;
  if (F && (!slot || !octave)) return invalid(fn, "NULL feature list");
  if (!g->h.slots_ok((int)F, slot)) return invalid(fn, "slot outside [0, point_capacity)");
  std::lock_guard<std::mutex> lk(g->m);
  if (int rc = obs_ready(g)) return rc;
  Arena* ar = &g->arena;
  int32_t *dKf, *dCand, *dSlot, *dMps, *dRed;
  uint8_t* dOct;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dKf, kf_slot, C));
    TRY(up_pack(a, &dCand, F, [&](int32_t* cand) {
      for (int c = 0; c < n_kf; c++)
        for (int f = offsets[c]; f < offsets[c + 1]; f++) cand[f] = c;
    }));
    TRY(up(a, &dSlot, slot, F));
    TRY(up(a, &dOct, octave, F));
    open_span(a);
    dMps = carve<int32_t>(a, C);
    dRed = carve<int32_t>(a, C);
    return close_span(a);
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  HIPCHK(flush(ar));
  HIPCHK(zero_span(ar));  // both counts
  launch_obs_culling(ar->stream, g->d, (int)F, dCand, dKf, dSlot, dOct, dMps, dRed);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(n_mps, mirror_of(ar, dMps), C * 4);
  std::memcpy(n_redundant, mirror_of(ar, dRed), C * 4);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_update_normal_depth(orbfe_obsgraph* g, int n, const int32_t* slot, const float* pos, const float* scale_factors,
                                                  int n_levels, float* normal, float* min_dist, float* max_dist, uint8_t* valid) {
  const char* fn = "obsgraph_update_normal_depth";
  if (!g || n < 0) return invalid(fn, "bad argument");
  if (const char* e = check_scale(scale_factors, n_levels)) return invalid(fn, e);
  if (n == 0) return ORBFE_OK;
  if (!slot || !pos || !normal || !min_dist || !max_dist || !valid) return invalid(fn, "NULL array");
  if (!g->h.slots_ok(n, slot)) return invalid(fn, "slot outside [0, point_capacity)");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.check_levels(n, slot, n_levels)) return invalid(fn, e);
  if (int rc = obs_ready(g)) return rc;
  return normal_depth_run(g, n, slot, pos, scale_factors, n_levels, normal, min_dist, max_dist, valid, nullptr);
}

extern "C" int orbfe_obsgraph_update_normal_depth_mappoints(orbfe_obsgraph* g, orbfe_mappoints* mp, int n, const int32_t* slot,
                                                            const float* scale_factors, int n_levels, uint8_t* valid) {
  const char* fn = "obsgraph_update_normal_depth_mappoints";
  if (!g || !mp || n < 0) return invalid(fn, "bad argument");
  if (const char* e = check_scale(scale_factors, n_levels)) return invalid(fn, e);
  if (mappoints_device(mp) != g->device) return invalid(fn, "the graph and the map-point table are on different devices");
  if (g->h.pointCap > orbfe_mappoints_capacity(mp)) return invalid(fn, "the graph has more point slots than the map-point table");
  if (n == 0) return ORBFE_OK;
  if (!slot) return invalid(fn, "NULL slot list");
  if (!g->h.slots_ok(n, slot)) return invalid(fn, "slot outside [0, point_capacity)");
  {  // a slot named twice would be rewritten by two waves
    std::vector<int32_t> sorted(slot, slot + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return invalid(fn, "a slot is named twice");
  }
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.check_levels(n, slot, n_levels)) return invalid(fn, e);
  MapPointsLock lock(mp);  // the table's own calls have completed and stay out for the scope
  if (lock.rc) return lock.rc;
  if (int rc = obs_ready(g)) return rc;
  return normal_depth_run(g, n, slot, nullptr, scale_factors, n_levels, nullptr, nullptr, nullptr, valid, lock.table);
}

// ---- the replays: pure host code (obsgraph_host.h) ----

extern "C" int orbfe_obsgraph_update_connections(int n, const int64_t* kf_id, const int32_t* weight, int64_t* ordered_id,
                                                 int32_t* ordered_weight, int* n_ordered, int64_t* connect_id, int32_t* connect_weight,
                                                 int* n_connect, int64_t* parent_id) {
  if (const char* e = obsgraph_update_connections(n, kf_id, weight, 15, ordered_id, ordered_weight, n_ordered, connect_id, connect_weight,
                                                  n_connect, parent_id))
    return invalid("obsgraph_update_connections", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_local_keyframes(int n, const int64_t* kf_id, const int32_t* weight, const uint8_t* bad, const int32_t* neigh_offsets,
                                              const int64_t* neigh_ids, const uint8_t* neigh_bad, const int32_t* child_offsets,
                                              const int64_t* child_ids, const uint8_t* child_bad, const int64_t* parent_id, int64_t* out_ids,
                                              int capacity, int* n_out, int64_t* ref_id) {
  bool over;
  if (const char* e = obsgraph_local_keyframes(n, kf_id, weight, bad, neigh_offsets, neigh_ids, neigh_bad, child_offsets, child_ids, child_bad,
                                               parent_id, out_ids, capacity, n_out, ref_id, &over))
    return over ? fail(ORBFE_ERR_CAPACITY, std::string("obsgraph_local_keyframes: ") + e) : invalid("obsgraph_local_keyframes", e);
  return ORBFE_OK;
}
