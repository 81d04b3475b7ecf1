// obsdesc.hip -- host side of the key frames' descriptors in the device observation graph and of the loop over them
// (include/orbfe.h: orbfe_obsgraph_*keyframe_descriptors*, orbfe_obsgraph_distinctive_descriptors*; kernel:
// k_obsdesc.hip).  Reference: MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333), which LocalMapping runs on
// every map point a new key frame touched (src/LocalMapping.cc: ProcessNewKeyFrame, CreateNewMapPoints, SearchInNeighbors).
//
// The descriptors live in a slab of their own, uint8 [kf_capacity][kf_desc_width][32], taken at the first set.  A key
// frame's descriptors never change in the reference, so there is no host copy of the bytes: the mirror (obsgraph_host.h)
// keeps the row count per kf slot, which is all the checks need, and the two set calls are the handle's only mutations
// that touch the device.  Otherwise the discipline is obsgraph.hip's: every operand is checked on the host, from the
// mirror, before anything is enqueued, and everything runs on the handle's one stream and is complete on return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "frame.h"
#include "host_internal.h"
#include "match_kernels.h"
#include "obsgraph_handle.h"
#include "obsgraph_host.h"
#include "obsgraph_kernels.h"

using namespace orbfe;

namespace {

const char* kNotEnabled = "key-frame descriptors are not enabled (orbfe_obsgraph_enable_keyframe_descriptors)";

// the device, the stream and the descriptors' slab (the handle locked, the store enabled)
int desc_ready(orbfe_obsgraph* g) {
  HIPCHK(arena_stream(&g->arena, g->device));
  if (!g->descTable.p) {
    HIPCHK(slab_get(g->device, (size_t)g->h.kfCap * (size_t)g->h.kfDescWidth * 32, &g->descTable));
    g->dd.desc = static_cast<const uint8_t*>(g->descTable.p);
    g->dd.width = g->h.kfDescWidth;
  }
  return ORBFE_OK;
}

uint8_t* desc_row(orbfe_obsgraph* g, int kf_slot) {
  return static_cast<uint8_t*>(g->descTable.p) + (size_t)kf_slot * (size_t)g->h.kfDescWidth * 32;
}

// table == NULL: the array form
int distinctive_run(orbfe_obsgraph* g, int n, const int32_t* slot, int32_t* best_kf_slot, int32_t* best_idx, uint8_t* desc, uint8_t* valid,
                    const MapPointsDevice* table) {
  const size_t q = (size_t)n;
  int maxCount = 0;
  for (int i = 0; i < n; i++) maxCount = std::max(maxCount, (int)g->h.meta[(size_t)slot[i]].count);
  // what comes back: valid always; the winners and the bytes where the caller asked (the winners lie between the two, so
  // they travel with the bytes).  What the kernel writes and nobody asked for is carved behind the span.
  const bool wantDesc = !table && desc, wantBest = best_kf_slot || best_idx || wantDesc;
  Arena* ar = &g->arena;
  int32_t *dSlot, *dKf = nullptr, *dIdx = nullptr;
  uint8_t *dValid, *dDesc = nullptr;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dSlot, slot, q));
    auto best = [&] { dKf = carve<int32_t>(a, q); dIdx = carve<int32_t>(a, q); };
    open_span(a);
    dValid = carve<uint8_t>(a, q);
    if (wantBest) best();
    if (wantDesc) dDesc = carve<uint8_t>(a, 32 * q);
    TRY(close_span(a));
    if (!wantBest) best();
    if (!table && !desc) dDesc = carve<uint8_t>(a, 32 * q);
    return hipSuccess;
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  HIPCHK(flush(ar));
  launch_obs_distinctive(ar->stream, g->d, g->dd, n, dSlot, maxCount, dKf, dIdx, dDesc, dValid, table);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const uint8_t* v = mirror_of(ar, dValid);
  std::memcpy(valid, v, q);
  if (!wantBest) return ORBFE_OK;
  const int32_t *hk = mirror_of(ar, dKf), *hi = mirror_of(ar, dIdx);
  const uint8_t* hd = wantDesc ? mirror_of(ar, dDesc) : nullptr;
  for (size_t i = 0; i < q; i++) {  // valid = 0 writes nothing
    if (!v[i]) continue;
    if (best_kf_slot) best_kf_slot[i] = hk[i];
    if (best_idx) best_idx[i] = hi[i];
    if (wantDesc) std::memcpy(desc + 32 * i, hd + 32 * i, 32);
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_obsgraph_enable_keyframe_descriptors(orbfe_obsgraph* g, int kf_desc_width) {
  const char* fn = "obsgraph_enable_keyframe_descriptors";
  if (!g) return obs_invalid(fn, "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  try {
    if (const char* e = g->h.enable_keyframe_descriptors(kf_desc_width)) return obs_invalid(fn, e);
  } catch (const std::bad_alloc&) {
    return fail(ORBFE_ERR_NOMEM, "out of memory");
  }
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_set_keyframe_descriptors(orbfe_obsgraph* g, int kf_slot, int n, const uint8_t* desc) {
  const char* fn = "obsgraph_set_keyframe_descriptors";
  if (!g) return obs_invalid(fn, "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.check_set_keyframe_descriptors(kf_slot, n, desc != nullptr)) return obs_invalid(fn, e);
  if (int rc = desc_ready(g)) return rc;
  const size_t bytes = (size_t)n * 32;
  if (bytes) {
    Arena* ar = &g->arena;
    uint8_t* staged;
    HIPCHK(arena_stage(ar, g->device, [&](Arena* a) { return up(a, &staged, desc, bytes); }));
    HIPCHK(send(ar, desc_row(g, kf_slot), staged, bytes));
    HIPCHK(hipStreamSynchronize(ar->stream));
  }
  g->h.descN[(size_t)kf_slot] = n;  // only now: a count always describes rows that have arrived
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_set_keyframe_descriptors_frame(orbfe_obsgraph* g, int kf_slot, const orbfe_frame* f) {
  const char* fn = "obsgraph_set_keyframe_descriptors_frame";
  if (!g || !f) return obs_invalid(fn, "NULL argument");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.check_set_keyframe_descriptors(kf_slot, f->n, f->n == 0 || f->ddesc != nullptr)) return obs_invalid(fn, e);
  if (f->device != g->device) return obs_invalid(fn, "the graph and the frame are on different devices");
  if (int rc = desc_ready(g)) return rc;
  const size_t bytes = (size_t)f->n * 32;
  if (bytes) {
    // the copy reads the frame on the handle's stream: frame_use() orders the arena's stream behind the frame's build
    UnsettledScope unsettled;
    HIPCHK(frame_use(&g->arena, f));
    HIPCHK(hipMemcpyAsync(desc_row(g, kf_slot), f->ddesc, bytes, hipMemcpyDeviceToDevice, g->arena.stream));
    HIPCHK(hipStreamSynchronize(g->arena.stream));  // complete on return: the frame may be released
    frames_settle();
  }
  g->h.descN[(size_t)kf_slot] = f->n;
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_get_keyframe_descriptors(orbfe_obsgraph* g, int kf_slot, uint8_t* desc_out, int32_t* n_out) {
  const char* fn = "obsgraph_get_keyframe_descriptors";
  if (!g || !desc_out || !n_out) return obs_invalid(fn, "NULL argument");
  std::lock_guard<std::mutex> lk(g->m);
  if (!g->h.kfDescWidth) return obs_invalid(fn, kNotEnabled);
  if (kf_slot < 0 || kf_slot >= g->h.kfCap) return obs_invalid(fn, "kf slot outside [0, kf_capacity)");
  const int n = g->h.descN[(size_t)kf_slot];
  if (n > 0) {  // (a count above 0 means the slab is there)
    const size_t bytes = (size_t)n * 32;
    if (int rc = desc_ready(g)) return rc;
    Arena* ar = &g->arena;
    uint8_t* got;
    auto stage = [&](Arena* a) { open_span(a); got = carve<uint8_t>(a, bytes); return close_span(a); };
    HIPCHK(arena_stage(ar, g->device, stage));
    HIPCHK(fetch(ar, got, desc_row(g, kf_slot), bytes));
    HIPCHK(hipStreamSynchronize(ar->stream));
    std::memcpy(desc_out, mirror_of(ar, got), bytes);
  }
  *n_out = n;
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_distinctive_descriptors(orbfe_obsgraph* g, int n, const int32_t* slot, int32_t* best_kf_slot, int32_t* best_idx,
                                                      uint8_t* desc, uint8_t* valid) {
  const char* fn = "obsgraph_distinctive_descriptors";
  if (!g || n < 0) return obs_invalid(fn, "bad argument");
  std::lock_guard<std::mutex> lk(g->m);
  if (!g->h.kfDescWidth) return obs_invalid(fn, kNotEnabled);
  if (n == 0) return ORBFE_OK;
  if (!slot || !best_kf_slot || !best_idx || !valid) return obs_invalid(fn, "NULL array");
  if (const char* e = g->h.check_distinctive(n, slot)) return obs_invalid(fn, e);
  if (int rc = obs_ready(g)) return rc;
  return distinctive_run(g, n, slot, best_kf_slot, best_idx, desc, valid, nullptr);
}

extern "C" int orbfe_obsgraph_distinctive_descriptors_mappoints(orbfe_obsgraph* g, orbfe_mappoints* mp, int n, const int32_t* slot,
                                                                int32_t* best_kf_slot, int32_t* best_idx, uint8_t* valid) {
  const char* fn = "obsgraph_distinctive_descriptors_mappoints";
  if (!g || !mp || n < 0) return obs_invalid(fn, "bad argument");
  if (mappoints_device(mp) != g->device) return obs_invalid(fn, "the graph and the map-point table are on different devices");
  if (g->h.pointCap > orbfe_mappoints_capacity(mp)) return obs_invalid(fn, "the graph has more point slots than the map-point table");
  std::lock_guard<std::mutex> lk(g->m);
  if (!g->h.kfDescWidth) return obs_invalid(fn, kNotEnabled);
  if (n == 0) return ORBFE_OK;
  if (!slot || !valid) return obs_invalid(fn, "NULL array");
  if (const char* e = g->h.check_distinctive(n, slot)) return obs_invalid(fn, e);
  {  // a slot named twice would be rewritten by two waves
    std::vector<int32_t> sorted(slot, slot + n);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return obs_invalid(fn, "a slot is named twice");
  }
  MapPointsLock lock(mp);  // the table's own calls have completed and stay out for the scope
  if (lock.rc) return lock.rc;
  if (int rc = obs_ready(g)) return rc;
  return distinctive_run(g, n, slot, best_kf_slot, best_idx, nullptr, valid, lock.table);
}
