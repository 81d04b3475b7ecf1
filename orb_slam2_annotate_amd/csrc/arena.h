// arena.h -- a device arena with its pinned mirror and stream, the thread's pinned staging buffer and the event pool: what
// a host file of csrc/ includes to run a call on a stream.  An arena has one of two kinds of owner:
//   the calling thread   a private arena + stream per device (the reference constructs stack-local ORBmatcher objects on
//                        three threads concurrently, src/LocalMapping.cc:261, src/LoopClosing.cc:294), so the entry
//                        points built on it are stateless and re-entrant
//   a handle             a member of the handle (orbfe_obsgraph, orbfe_kfdb), used with the handle locked: the handle's
//                        calls run on its own stream, whichever thread makes them
//
// Two ways in, each of which begins the arena anew (what an earlier call left in it is gone); `device, &ar` names the
// calling thread's arena, `&own, device` one that a handle owns:
//   arena_stage(device, &ar, stage)    a call that carves: up() / up_pack() / up_fill() / carve() inside `stage`, then
//   arena_stage(&own, device, stage)   flush(), the launches, down_span() / down_range(), a synchronisation, mirror_of()
//   arena_stream(device, &ar)          the stream alone
//   arena_stream(&own, device)
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
  bool sizing = false;  // arena_stage()'s first pass: carve() only advances `used`, the up*() calls write nothing
  struct OutSpan {
    size_t lo = 0, hi = 0;  // arena offsets: the start of the first output, the end of the last (not rounded up)
  } out;                    // open_span() / close_span() / down_span()
  ~Arena() {  // (thread exit, or the owning handle's end; the buffers free themselves behind this, on the device set here)
    if (device >= 0) {
      (void)hipSetDevice(device);
      if (stream) (void)hipStreamDestroy(stream);
    }
  }
};

// begin an arena with room for `bytes` -- the calling thread's of `device`, or `own` (its stream is made on `device` by the
// first begin): behind arena_stage / arena_stream, which are what callers use
hipError_t arena_begin(int device, size_t bytes, Arena** out);
hipError_t arena_begin_owned(Arena* own, int device, size_t bytes);

template <typename T>
T* carve(Arena* a, size_t n) {
  size_t off = (a->used + 255) & ~(size_t)255;
  a->used = off + n * sizeof(T);
  return reinterpret_cast<T*>(reinterpret_cast<uintptr_t>(a->base.p) + off);
}

// the pinned mirror covers arena offsets [0, upto); what earlier up() calls of this call staged is kept
hipError_t grow_mirror(Arena* a, size_t upto);
inline void mark_dirty(Arena* a, size_t off, size_t bytes) {
  const bool none = a->dirtyHi == a->dirtyLo;
  if (none || off < a->dirtyLo) a->dirtyLo = off;
  if (none || off + bytes > a->dirtyHi) a->dirtyHi = off + bytes;
}
// the one body of staging: fill(h) writes the `bytes` of the array carved at `d` at their place h in the mirror.  Not in the
// sizing pass and not for an empty array; h is good inside `fill` only, the next grow_mirror() may move the mirror
template <typename Fill>
hipError_t stage_bytes(Arena* a, const void* d, size_t bytes, Fill&& fill) {
  if (bytes == 0 || a->sizing) return hipSuccess;
  const size_t off = (size_t)(static_cast<const uint8_t*>(d) - a->base);
  TRY(grow_mirror(a, off + bytes));
  fill(a->hmirror + off);
  mark_dirty(a, off, bytes);
  return hipSuccess;
}
// host data for an array carved earlier in this call: for blocks of device addresses, which are known only once everything
// is carved but must lie among the uploads
template <typename T>
hipError_t put(Arena* a, T* d, const T* h, size_t n) {
  return stage_bytes(a, d, n * sizeof(T), [&](uint8_t* m) { std::memcpy(m, h, n * sizeof(T)); });
}
template <typename T>
hipError_t up(Arena* a, T** d, const T* h, size_t n) {
  *d = carve<T>(a, n ? n : 1);
  return put(a, *d, h, n);
}
// a device array of n elements that the call packs in place: fill(T* h) writes the n elements in the mirror, which saves
// the host copy a finished array handed to up() would cost
template <typename T, typename Fill>
hipError_t up_pack(Arena* a, T** d, size_t n, Fill&& fill) {
  *d = carve<T>(a, n ? n : 1);
  return stage_bytes(a, *d, n * sizeof(T), [&](uint8_t* m) { fill(reinterpret_cast<T*>(m)); });
}
// a device array of n elements whose bytes all start as `byteValue`: filled in the mirror, so it travels with the one
// host-to-device copy of the call instead of costing a fill kernel of its own
template <typename T>
hipError_t up_fill(Arena* a, T** d, size_t n, int byteValue) {
  const size_t bytes = (n ? n : 1) * sizeof(T);
  *d = carve<T>(a, n ? n : 1);
  return stage_bytes(a, *d, bytes, [&](uint8_t* m) { std::memset(m, byteValue, bytes); });
}
// results: ONE device-to-host copy of the arena range [first, last) into the pinned mirror (same offsets), to be read
// through mirror_of() after the stream is synchronised -- instead of one pageable copy per output array
hipError_t down_range(Arena* a, const void* first, const void* last);
// The outputs of a call, carved next to each other: `stage` opens the arena's span before its first output carve and closes
// it after its last, down_span() is then the one copy back.  The span is what was carved, so an output added inside it
// travels without anyone restating where the range ends.
inline void open_span(Arena* a) { a->out.lo = (a->used + 255) & ~(size_t)255; }  // where carve() puts the next array
inline hipError_t close_span(Arena* a) {
  a->out.hi = a->used;
  return a->sizing ? hipSuccess : grow_mirror(a, a->out.hi);  // the mirror reaches the outputs before flush() reads from it
}
inline hipError_t down_span(Arena* a) { return down_range(a, a->base + a->out.lo, a->base + a->out.hi); }
inline size_t span_bytes(const Arena* a) { return a->out.hi - a->out.lo; }
inline hipError_t zero_span(Arena* a) { return hipMemsetAsync(a->base + a->out.lo, 0, span_bytes(a), a->stream); }  // ONE fill
template <typename T>
const T* mirror_of(Arena* a, const T* d) {
  return reinterpret_cast<const T*>(a->hmirror + (reinterpret_cast<const uint8_t*>(d) - a->base));
}
// The few copies whose other end is a slab, not the arena, each ONE copy on the arena's stream.  fetch: n elements of device
// memory at `src` into the mirror, at the place of the array carved at `at`, to be read through mirror_of() after a
// synchronisation; the place must lie inside the closed output span, which the mirror reaches.  send: the n elements that
// up() / up_pack() staged for the array carved at `at`, from the mirror to the device address `dst`; a call that only sends
// does not flush(), so the bytes travel once.  Either fails with hipErrorInvalidValue, nothing enqueued, on another place.
template <typename T>
hipError_t fetch(Arena* a, T* at, const T* src, size_t n) {
  const size_t off = (size_t)(reinterpret_cast<const uint8_t*>(at) - a->base);
  if (off < a->out.lo || off + n * sizeof(T) > a->out.hi) return hipErrorInvalidValue;
  return hipMemcpyAsync(a->hmirror + off, src, n * sizeof(T), hipMemcpyDeviceToHost, a->stream);
}
template <typename T>
hipError_t send(Arena* a, T* dst, const T* at, size_t n) {
  const size_t off = (size_t)(reinterpret_cast<const uint8_t*>(at) - a->base);
  if (off < a->dirtyLo || off + n * sizeof(T) > a->dirtyHi) return hipErrorInvalidValue;
  return hipMemcpyAsync(dst, a->hmirror + off, n * sizeof(T), hipMemcpyHostToDevice, a->stream);
}
// one H2D copy for everything staged since arena_begin(); call before the first kernel launch.  Whole 256-byte lines
// travel (a copy that ends inside a line costs a microsecond more): carve() starts every array on a line and arena_begin()
// reserves whole lines, so the tail of the last line belongs to no array
hipError_t flush(Arena* a);

// Stages a call: runs `stage` -- the up*() / carve() calls of the call -- twice, first on a sizing arena that
// only counts, then on the arena that begin(bytes, out) begins with exactly what the first pass carved: the size
// cannot drift from the carving.  `stage` must carve the same sizes in both passes: one that does not fails the call
// with hipErrorInvalidValue before anything is enqueued.
template <typename F, typename Begin>
hipError_t stage_two_pass(Arena** out, F&& stage, Begin&& begin) {
  Arena sizing;
  sizing.sizing = true;
  hipError_t e = stage(&sizing);
  if (e == hipSuccess) e = begin(sizing.used, out);
  if (e == hipSuccess) e = stage(*out);
  if (e == hipSuccess && (*out)->used != sizing.used) e = hipErrorInvalidValue;
  return e;
}
// on the calling thread's arena of `device`
template <typename F>
hipError_t arena_stage(int device, Arena** out, F&& stage) {
  return stage_two_pass(out, stage, [device](size_t bytes, Arena** o) { return arena_begin(device, bytes, o); });
}
// on an arena that a handle owns (the handle locked)
template <typename F>
hipError_t arena_stage(Arena* own, int device, F&& stage) {
  Arena* ar;
  return stage_two_pass(&ar, stage, [own, device](size_t bytes, Arena** o) { *o = own; return arena_begin_owned(own, device, bytes); });
}
// the stream alone -- (*out)->stream, own->stream -- for a call that carves nothing
hipError_t arena_stream(int device, Arena** out);
inline hipError_t arena_stream(Arena* own, int device) { return arena_begin_owned(own, device, 0); }

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
