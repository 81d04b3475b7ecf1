// arena.hip -- the state behind arena.h: the thread-local arenas and staging buffer, the begin of an arena whoever owns it,
// the process-wide pool of device slabs (host_internal.h: slab_get / slab_put) and events, and the two test hooks on the
// calling thread's stream.
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"

namespace orbfe {

namespace {
thread_local std::map<int, Arena> t_arenas;
thread_local Staging t_staging;
}  // namespace

// Reserve `bytes` up front (sum of all buffers of a call), then carve.  Whose arena it is makes no difference here; the
// device is current.
static hipError_t begin_on(Arena& a, int device, size_t bytes) {
  hipError_t err;
  bytes = (bytes + 255) & ~(size_t)255;
  if (a.device < 0) {
    a.device = device;
    err = hipStreamCreateWithFlags(&a.stream, hipStreamNonBlocking);
    if (err != hipSuccess) { a.device = -1; return err; }
  }
  if (bytes > a.base.cap) {
    err = a.base.try_alloc(bytes + bytes / 2 + (1u << 20));
    if (err != hipSuccess) return err;
  }
  a.used = 0;
  a.dirtyLo = a.dirtyHi = 0;
  a.out = {};
  return hipSuccess;
}

hipError_t arena_begin_owned(Arena* own, int device, size_t bytes) {
  const hipError_t err = hipSetDevice(device);
  return err != hipSuccess ? err : begin_on(*own, device, bytes);
}
hipError_t arena_begin(int device, size_t bytes, Arena** out) {
  hipError_t err = hipSetDevice(device);
  if (err != hipSuccess) return err;
  Arena& a = t_arenas[device];
  err = begin_on(a, device, bytes);
  if (err == hipSuccess) *out = &a;
  return err;
}

hipError_t arena_stream(int device, Arena** out) { return arena_begin(device, 0, out); }

hipError_t grow_mirror(Arena* a, size_t upto) {
  if (upto <= a->hmirror.cap) return hipSuccess;
  PinBuf<uint8_t> nh;
  hipError_t e = nh.try_alloc(upto + upto / 2 + (1u << 16));
  if (e != hipSuccess) return e;
  if (a->hmirror && a->dirtyHi > a->dirtyLo) std::memcpy(nh + a->dirtyLo, a->hmirror + a->dirtyLo, a->dirtyHi - a->dirtyLo);
  a->hmirror = std::move(nh);
  return hipSuccess;
}
hipError_t down_range(Arena* a, const void* first, const void* last) {
  const size_t lo = (size_t)(reinterpret_cast<const uint8_t*>(first) - a->base);
  const size_t hi = (size_t)(reinterpret_cast<const uint8_t*>(last) - a->base);
  hipError_t e = grow_mirror(a, hi);
  if (e != hipSuccess) return e;
  return hipMemcpyAsync(a->hmirror + lo, a->base + lo, hi - lo, hipMemcpyDeviceToHost, a->stream);
}
hipError_t flush(Arena* a) {
  if (a->dirtyHi == a->dirtyLo) return hipSuccess;
  const size_t hi = (a->dirtyHi + 255) & ~(size_t)255;
  hipError_t e = grow_mirror(a, hi);
  if (e == hipSuccess) e = hipMemcpyAsync(a->base + a->dirtyLo, a->hmirror + a->dirtyLo, hi - a->dirtyLo, hipMemcpyHostToDevice, a->stream);
  a->dirtyLo = a->dirtyHi = 0;
  return e;
}

Staging& thread_staging() { return t_staging; }
hipError_t staging_reserve(size_t bytes) {
  if (t_staging.isPending) {  // (normally long done: the copy took microseconds, the caller's next call comes later)
    hipError_t e = hipEventSynchronize(t_staging.pending);
    if (e != hipSuccess) return e;
    t_staging.isPending = false;
  }
  return bytes <= t_staging.h.cap ? hipSuccess : t_staging.h.try_alloc(bytes + bytes / 2 + (1u << 16));
}
hipError_t staging_mark_pending(hipStream_t s) {
  if (!t_staging.pending) {
    hipError_t e = hipEventCreateWithFlags(&t_staging.pending, hipEventDisableTiming);
    if (e != hipSuccess) return e;
  }
  hipError_t e = hipEventRecord(t_staging.pending, s);
  if (e == hipSuccess) t_staging.isPending = true;
  return e;
}

namespace {
// Slabs (host_internal.h: resident frames, map-point tables, the key-frame database's arrays) and events of released frames are kept
// for the next upload: hipMalloc / hipFree cost tens of microseconds and hipFree waits for the whole device -- in a live
// system every key-frame insertion would stall the extractor's streams.
struct DevicePool {
  std::mutex m;
  std::vector<Slab> slabs;
  std::vector<std::pair<int, hipEvent_t>> events;
  static constexpr size_t kKeepSlabs = 80, kKeepEvents = 256;
  ~DevicePool() {}  // (process exit: the runtime reclaims device memory; no HIP calls from static destructors)
};
DevicePool g_pool;
}  // namespace

hipError_t slab_get(int device, size_t bytes, Slab* out) {
  {
    std::lock_guard<std::mutex> lk(g_pool.m);
    auto& v = g_pool.slabs;
    int best = -1;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i].device == device && v[i].cap >= bytes && v[i].cap <= 4 * bytes + (1u << 16) && (best < 0 || v[i].cap < v[(size_t)best].cap))
        best = (int)i;
    if (best >= 0) {
      *out = v[(size_t)best];
      v.erase(v.begin() + best);
      return hipSuccess;
    }
  }
  const size_t want = (bytes + (1u << 16) - 1) & ~(size_t)((1u << 16) - 1);  // 64 KB classes: users of similar size share slabs
  *out = Slab{};
  hipError_t e = hipMalloc(&out->p, want);
  if (e == hipSuccess) { out->cap = want; out->device = device; } else out->p = nullptr;
  return e;
}
void slab_put(Slab* s) {
  if (!s->p) return;
  bool kept = false;
  {
    std::lock_guard<std::mutex> lk(g_pool.m);
    if (g_pool.slabs.size() < DevicePool::kKeepSlabs) { g_pool.slabs.push_back(*s); kept = true; }
  }
  if (!kept) (void)hipFree(s->p);
  *s = Slab{};
}
hipError_t event_get(int device, hipEvent_t* e) {
  {
    std::lock_guard<std::mutex> lk(g_pool.m);
    auto& v = g_pool.events;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i].first == device) { *e = v[i].second; v.erase(v.begin() + (long)i); return hipSuccess; }
  }
  return hipEventCreateWithFlags(e, hipEventDisableTiming);
}
void event_put(int device, hipEvent_t e) {
  if (!e) return;
  {
    std::lock_guard<std::mutex> lk(g_pool.m);
    if (g_pool.events.size() < DevicePool::kKeepEvents) { g_pool.events.push_back({device, e}); return; }
  }
  (void)hipEventDestroy(e);
}

}  // namespace orbfe

using namespace orbfe;

// ---- test hook (tests/stream_order.py): hold back / query the calling thread's matcher stream on `device` ----
extern "C" int orbfe_debug_stall_thread_stream(int device, int usec) {
  if (usec < 0 || usec > 1000000) return fail(ORBFE_ERR_INVALID, "debug_stall: usec must be 0 .. 1000000");
  Arena* ar;
  hipError_t err = arena_stream(device, &ar);
  if (err != hipSuccess) return fail(hip_status(err), std::string("debug_stall: ") + hipGetErrorString(err));
  return orbfe_debug_stall_launch_(ar->stream, usec);
}

extern "C" int orbfe_debug_thread_stream_idle(int device) {
  Arena* ar;
  hipError_t err = arena_stream(device, &ar);
  if (err != hipSuccess) return fail(hip_status(err), std::string("debug_stream_idle: ") + hipGetErrorString(err));
  return orbfe_debug_stream_idle_(ar->stream);
}
