// mappoints.hip -- C-ABI entry points of the device map-point table (include/orbfe.h: orbfe_mappoints_*) and MapPointsLock
// (host_internal.h), the one way another host file reaches the table.  What projects or searches the points is
// mappoints_search.hip.
#include <hip/hip_runtime.h>

#include <cstring>
#include <mutex>
#include <new>
#include <string>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "mappoints_host.h"
#include "match_kernels.h"

using namespace orbfe;

// ---------------------------------------------------------------------------------------------
// Device-resident map points (include/orbfe.h: orbfe_mappoints).  One slab from the pool holds the table; an update is one
// staged copy (arena.h: arena_stage) and one scatter launch on the calling thread's stream, complete on return.  The
// argument checks, the slab layout and the interleaving of an update's records are mappoints_host.h (no device needed:
// tests/cpp/mappoints_host_san.cpp runs them under the sanitizers).
// ---------------------------------------------------------------------------------------------
struct orbfe_mappoints {
  int device = 0, capacity = 0;
  std::mutex m;  // a handle serialises its own calls
  Slab slab;     // empty until the first call that needs the device
  MapPointsDevice d{};
};

namespace {
// the table's slab, every slot bad until it is updated; enqueued on the arena's stream
hipError_t mappoints_ready(orbfe_mappoints* mp, Arena* ar) {
  if (mp->slab.p) return hipSuccess;
  const MapPointsLayout L = mappoints_layout(mp->capacity);
  TRY(slab_get(mp->device, L.total, &mp->slab));
  uint8_t* b = static_cast<uint8_t*>(mp->slab.p);
  mp->d.rec = reinterpret_cast<float4*>(b + L.oRec); mp->d.desc = b + L.oDesc; mp->d.flags = b + L.oFlags;
  hipError_t e = hipMemsetAsync(b, 0, L.oFlags, ar->stream);
  if (e == hipSuccess) e = hipMemsetAsync(mp->d.flags, ORBFE_MP_BAD, (size_t)mp->capacity, ar->stream);
  // complete before the handle counts as ready: another thread's stream may be the next to read the table
  if (e == hipSuccess) e = hipStreamSynchronize(ar->stream);
  if (e != hipSuccess) { slab_put(&mp->slab); mp->d = MapPointsDevice{}; }
  return e;
}
}  // namespace

extern "C" int orbfe_mappoints_create(int device, int capacity, orbfe_mappoints** out) {
  if (const char* e = mappoints_check_create(capacity, out)) return fail(ORBFE_ERR_INVALID, std::string("mappoints_create: ") + e);
  *out = nullptr;
  if (device < 0) return fail(ORBFE_ERR_INVALID, "mappoints_create: negative device");
  orbfe_mappoints* mp = new (std::nothrow) orbfe_mappoints();
  if (!mp) return fail(ORBFE_ERR_NOMEM, "out of memory");
  mp->device = device; mp->capacity = capacity;
  *out = mp;
  return ORBFE_OK;
}

extern "C" void orbfe_mappoints_destroy(orbfe_mappoints* mp) {
  if (!mp) return;
  if (mp->slab.p) {  // (every call on the table has completed on return: nothing can still read the slab)
    (void)hipSetDevice(mp->device);
    slab_put(&mp->slab);
  }
  delete mp;
}

extern "C" int orbfe_mappoints_capacity(const orbfe_mappoints* mp) { return mp ? mp->capacity : fail(ORBFE_ERR_INVALID, "mappoints_capacity: NULL table"); }

extern "C" int orbfe_mappoints_update(orbfe_mappoints* mp, int n, const int32_t* slot, const float* pos, const float* normal,
                                      const float* min_dist, const float* max_dist, const uint8_t* desc, const uint8_t* flags) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "mappoints_update: NULL table");
  if (const char* e = mappoints_check_update(mp->capacity, n, slot, pos, normal, min_dist, max_dist, flags))
    return fail(ORBFE_ERR_INVALID, std::string("mappoints_update: ") + e);
  if (n == 0) return ORBFE_OK;
  std::lock_guard<std::mutex> lk(mp->m);
  Arena* ar;
  int32_t* dslot;
  float4* drec;
  uint8_t *dflags, *ddesc = nullptr;
  auto stage = [&](Arena* a) -> hipError_t {  // in the order the scatter kernel reads: slots | records | flags | descriptors
    TRY(up(a, &dslot, slot, (size_t)n));
    TRY(up_pack(a, &drec, 2 * (size_t)n, [&](float4* h) { mappoints_pack_records(&h->x, n, pos, normal, min_dist, max_dist); }));
    TRY(up(a, &dflags, flags, (size_t)n));
    if (desc) TRY(up(a, &ddesc, desc, 32 * (size_t)n));
    return hipSuccess;
  };
  HIPCHK(arena_stage(mp->device, &ar, stage));
  HIPCHK(mappoints_ready(mp, ar));
  HIPCHK(flush(ar));
  launch_mappoints_scatter(ar->stream, mp->d, n, dslot, drec, dflags, ddesc);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ar->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_mappoints_descriptors(orbfe_mappoints* mp, int n_slots, const int32_t* slot, uint8_t* desc_out) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "mappoints_descriptors: NULL table");
  if (const char* e = mappoints_check_slots(mp->capacity, n_slots, slot)) return fail(ORBFE_ERR_INVALID, std::string("mappoints_descriptors: ") + e);
  if (n_slots > 0 && !desc_out) return fail(ORBFE_ERR_INVALID, "mappoints_descriptors: NULL output");
  if (n_slots == 0) return ORBFE_OK;
  const size_t q = (size_t)n_slots;
  std::lock_guard<std::mutex> lk(mp->m);
  Arena* ar;
  int32_t* dslot;
  uint8_t* dout = nullptr;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dslot, slot, q));
    dout = carve<uint8_t>(a, 32 * q);
    return a->sizing ? hipSuccess : grow_mirror(a, (size_t)(dout + 32 * q - a->base.p));
  };
  HIPCHK(arena_stage(mp->device, &ar, stage));
  HIPCHK(mappoints_ready(mp, ar));
  HIPCHK(flush(ar));
  launch_mappoints_read_descriptors(ar->stream, mp->d, n_slots, dslot, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, dout, dout + 32 * q));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(desc_out, mirror_of(ar, dout), 32 * q);
  return ORBFE_OK;
}

namespace orbfe {
bool pose_ok(const orbfe_camera_pose* p) { return p && p->n_levels >= 1 && p->n_levels <= ORBFE_MAX_LEVELS * 4; }
int mappoints_device(const orbfe_mappoints* mp) { return mp->device; }

// host_internal.h: holds the handle's serialisation for a scope, with the table on the device
MapPointsLock::MapPointsLock(orbfe_mappoints* mp) {
  mp->m.lock();
  Arena* ar;
  hipError_t e = arena_stream(mp->device, &ar);
  if (e == hipSuccess) e = mappoints_ready(mp, ar);
  if (e != hipSuccess) {
    mp->m.unlock();
    rc = fail(hip_status(e), std::string("mappoints: ") + hipGetErrorString(e));
    return;
  }
  held = mp;
  table = &mp->d;
  device = mp->device;
}
MapPointsLock::~MapPointsLock() {
  if (held) held->m.unlock();
}
}  // namespace orbfe
