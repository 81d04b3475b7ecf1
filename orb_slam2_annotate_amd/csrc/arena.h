// arena.h -- the calling thread's device arena with its pinned mirror and stream, the thread's pinned staging buffer and the
// event pool: what a host file of csrc/ includes to run a call on the thread's matcher stream.  Every thread owns a private
// arena + stream per device (the reference constructs stack-local ORBmatcher objects on three threads concurrently,
// src/LocalMapping.cc:261, src/LoopClosing.cc:294), so the entry points built on it are stateless and re-entrant.
//
// Three ways in, each of which begins the arena anew (what an earlier call of the thread left in it is gone):
//   arena_stage(device, &ar, stage)    a call that carves: up() / up_fill() / carve() inside `stage`, then flush(), the
//                                      launches, down_range(), a synchronisation, mirror_of()
//   arena_scratch(device, bytes, &ar)  one block [0, bytes) of ar->base with ar->hmirror grown to match, laid out by the caller
//   arena_stream(device, &ar)          ar->stream alone
// State and the non-templates: arena.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>

#include "host_internal.h"

// (in a function that returns hipError_t)
#define TRY(expr)                      \
  do {                                 \
    hipError_t _e = (expr);            \
    if (_e != hipSuccess) return _e;   \
  } while (0)

namespace orbfe {

struct Arena {
  int device = -1;
  hipStream_t stream = nullptr;
  DevBuf<uint8_t> base;
  size_t used = 0;
  // pinned mirror of the uploaded part of the arena: up() only copies into it, flush() sends the whole
  // dirty range in ONE host-to-device copy before the first kernel of the call
  PinBuf<uint8_t> hmirror;
  size_t dirtyLo = 0, dirtyHi = 0;
  bool sizing = false;  // arena_stage()'s first pass: carve() only advances `used`, up() / up_fill() copy nothing
  ~Arena() {  // (thread exit; the buffers free themselves behind this, on the device set here)
    if (device >= 0) {
      (void)hipSetDevice(device);
      if (stream) (void)hipStreamDestroy(stream);
    }
  }
};

// begins the arena with room for `bytes`: behind arena_stage / arena_scratch / arena_stream, which are what callers use
hipError_t arena_begin(int device, size_t bytes, Arena** out);

template <typename T>
T* carve(Arena* a, size_t n) {
  size_t off = (a->used + 255) & ~(size_t)255;
  a->used = off + n * sizeof(T);
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(a->base.p) + off);
}

// the pinned mirror covers arena offsets [0, upto); what earlier up() calls of this call staged is kept
hipError_t grow_mirror(Arena* a, size_t upto);
inline void mark_dirty(Arena* a, size_t off, size_t bytes) {
  if (a->dirtyHi == a->dirtyLo) { a->dirtyLo = off; a->dirtyHi = off + bytes; }
  else {
    if (off < a->dirtyLo) a->dirtyLo = off;
    if (off + bytes > a->dirtyHi) a->dirtyHi = off + bytes;
  }
}
// host data for an array carved earlier in this call: for blocks of device addresses, which are known only once everything
// is carved but must lie among the uploads
template <typename T>
hipError_t put(Arena* a, T* d, const T* h, size_t n) {
  if (n == 0 || a->sizing) return hipSuccess;
  const size_t off = (size_t)(reinterpret_cast<uint8_t*>(d) - a->base), bytes = n * sizeof(T);
  hipError_t e = grow_mirror(a, off + bytes);
  if (e != hipSuccess) return e;
  std::memcpy(a->hmirror + off, h, bytes);
  mark_dirty(a, off, bytes);
  return hipSuccess;
}
template <typename T>
hipError_t up(Arena* a, T** d, const T* h, size_t n) {
  *d = carve<T>(a, n ? n : 1);
  return put(a, *d, h, n);
}
// a device array of n elements whose bytes all start as `byteValue`: filled in the mirror, so it travels with the one
// host-to-device copy of the call instead of costing a fill kernel of its own
template <typename T>
hipError_t up_fill(Arena* a, T** d, size_t n, int byteValue) {
  *d = carve<T>(a, n ? n : 1);
  if (a->sizing) return hipSuccess;
  const size_t off = (size_t)(reinterpret_cast<uint8_t*>(*d) - a->base), bytes = (n ? n : 1) * sizeof(T);
  hipError_t e = grow_mirror(a, off + bytes);
  if (e != hipSuccess) return e;
  std::memset(a->hmirror + off, byteValue, bytes);
  mark_dirty(a, off, bytes);
  return hipSuccess;
}
// results: ONE device-to-host copy of the arena range [first, last) into the pinned mirror (same offsets), to be read
// through mirror_of() after the stream is synchronised -- instead of one pageable copy per output array
hipError_t down_range(Arena* a, const void* first, const void* last);
template <typename T>
const T* mirror_of(Arena* a, const T* d) {
  return reinterpret_cast<const T*>(a->hmirror + (reinterpret_cast<const uint8_t*>(d) - a->base));
}
// one H2D copy for everything up() staged since arena_begin(); call before the first kernel launch.  Whole 256-byte lines
// travel (a copy that ends inside a line costs a microsecond more): carve() starts every array on a line and arena_begin()
// reserves whole lines, so the tail of the last line belongs to no array
hipError_t flush(Arena* a);

// Stages a call: runs `stage` -- the up() / up_fill() / carve() calls of the call -- twice, first on a sizing arena that
// only counts, then on the calling thread's arena of `device`, begun with exactly what the first pass carved: the size
// cannot drift from the carving.  `stage` must carve the same sizes in both passes: one that does not fails the call
// with hipErrorInvalidValue before anything is enqueued.
template <typename F>
hipError_t arena_stage(int device, Arena** out, F&& stage) {
  Arena sizing;
  sizing.sizing = true;
  hipError_t e = stage(&sizing);
  if (e == hipSuccess) e = arena_begin(device, sizing.used, out);
  if (e == hipSuccess) e = stage(*out);
  if (e == hipSuccess && (*out)->used != sizing.used) e = hipErrorInvalidValue;
  return e;
}
// one block [0, bytes) of the calling thread's arena on `device`, (*out)->base, and as much of its pinned mirror,
// (*out)->hmirror: the caller fills the mirror, copies, launches and copies back on (*out)->stream, and synchronises before
// it returns
hipError_t arena_scratch(int device, size_t bytes, Arena** out);
// the calling thread's stream on `device`, (*out)->stream, for a call that carves nothing
hipError_t arena_stream(int device, Arena** out);

// Pinned staging of the calling thread for copies whose destination is a slab, not the arena (frame builds,
// orbfe_frame_set_featvec): the call packs what travels in the slab's own layout and sends it in ONE
// host-to-device copy.  Everything else stages through the arena (up() / flush() / down_range()).
struct Staging {
  PinBuf<uint8_t> h;
  hipEvent_t pending = nullptr;  // an asynchronous copy OUT of the buffer that nobody waited for (orbfe_frame_upload): the
  bool isPending = false;        // next use of the buffer waits for it first
  ~Staging() {
    if (pending) (void)hipEventDestroy(pending);
  }
};
Staging& thread_staging();  // the calling thread's
hipError_t staging_reserve(size_t bytes);
// an asynchronous copy out of the staging buffer was enqueued on `s` and nobody waits for it: the next staging_reserve() does
hipError_t staging_mark_pending(hipStream_t s);

// events of released frames are kept for the next upload, as the slabs are (host_internal.h: slab_get / slab_put)
hipError_t event_get(int device, hipEvent_t* e);
void event_put(int device, hipEvent_t e);

}  // namespace orbfe
