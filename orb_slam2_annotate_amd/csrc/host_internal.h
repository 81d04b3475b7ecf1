// host_internal.h -- what one host translation unit of csrc/ defines for another.  The defining file and every user
// include it, so a signature that drifts is a compile error (the functions are extern "C": a hand-copied prototype would
// link whatever its parameters say).  tests/test_host_internal_header.py keeps prototypes out of the sources and dead
// entries out of this list.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "kernels.h"

namespace orbfe {
// runtime.hip: sets the text orbfe_last_error() returns on the calling thread; returns `code`
int fail(int code, const std::string& msg);
// the one status rule: out of memory answers ORBFE_ERR_NOMEM, every other HIP error ORBFE_ERR_HIP
inline int hip_status(hipError_t e) { return e == hipErrorOutOfMemory ? ORBFE_ERR_NOMEM : ORBFE_ERR_HIP; }
}  // namespace orbfe

// in a function that returns an ORBFE_* status
#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t _e = (expr);                                                                   \
    if (_e != hipSuccess)                                                                     \
      return orbfe::fail(orbfe::hip_status(_e), std::string(#expr) + ": " + hipGetErrorString(_e)); \
  } while (0)

namespace orbfe {
// How a call of `frames` frames is cut into S sub-batches of `per` consecutive frames (the last one may be shorter,
// and trailing ones empty): sub-batch i on its own stream, or -- lanes -- all of them on three shared lane streams.
struct SubSplit {
  int frames = 0, S = 0, per = 0;
  bool lanes = false;
  // frames [*f0, *f0 + *n) of sub-batch i; false behind the last sub-batch that has frames
  bool range(int i, int* f0, int* n) const {
    *f0 = i * per;
    *n = frames - *f0 < per ? frames - *f0 : per;
    return i < S && *n > 0;
  }
  bool operator==(const SubSplit& o) const { return frames == o.frames && S == o.S && per == o.per && lanes == o.lanes; }
};

// An owned array of T in device memory (kPinned: in page-locked host memory); converts to T* for launch sites.
template <typename T, bool kPinned = false>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;  // elements asked for by the alloc() that made p
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) { reset(); p = o.p; cap = o.cap; o.p = nullptr; o.cap = 0; }
    return *this;
  }
  ~DevBuf() { reset(); }
  void reset() {
    if (p) (void)(kPinned ? hipHostFree(p) : hipFree(p));
    p = nullptr;
    cap = 0;
  }
  // frees what it holds first; at least one element.  try_alloc: for helpers that pass the HIP error on
  hipError_t try_alloc(size_t n) {
    reset();
    const size_t bytes = (n ? n : 1) * sizeof(T);
    const hipError_t e = kPinned ? hipHostMalloc((void**)&p, bytes, hipHostMallocDefault) : hipMalloc((void**)&p, bytes);
    if (e == hipSuccess) cap = n;
    else p = nullptr;
    return e;
  }
  int alloc(size_t n) {
    HIPCHK(try_alloc(n));
    return ORBFE_OK;
  }
  // grow-only: room for `need` elements, or a fresh array of `grown` (the caller's growth policy); the old contents are
  // dropped, so whatever may still read them must have finished
  int reserve(size_t need, size_t grown) { return need <= cap ? ORBFE_OK : alloc(grown); }
  int upload(const T* src, size_t n) {
    int rc = alloc(n);
    if (rc) return rc;
    if (n) HIPCHK(hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice));
    return ORBFE_OK;
  }
  int upload(const std::vector<T>& v) { return upload(v.data(), v.size()); }
  operator T*() const { return p; }
};
template <typename T>
using PinBuf = DevBuf<T, true>;

// arena.hip: device slabs of released frames / map-point tables / key-frame databases, kept for the next one -- hipMalloc /
// hipFree cost tens of microseconds and hipFree waits for the whole device.  slab_get: the smallest kept slab of `device` with
// bytes <= cap <= 4 * bytes + 64 KiB, else a new one of the next 64 KiB class; slab_put: back to the pool (p = NULL after)
struct Slab {
  void* p = nullptr;
  size_t cap = 0;  // bytes
  int device = 0;
};
hipError_t slab_get(int device, size_t bytes, Slab* out);
void slab_put(Slab* s);

// ---- mappoints.hip (struct orbfe_mappoints lives there) ----
bool pose_ok(const orbfe_camera_pose* p);
// the device a table was created for (fixed at create: no lock, no device call)
int mappoints_device(const orbfe_mappoints* mp);
// The one way another host file reaches a table: takes the handle's serialisation and makes the table ready on the device,
// for the scope.  rc != ORBFE_OK: nothing is held and the error text is set.  The holder's work on the table has completed
// (its stream is synchronised) before the scope ends.
struct MapPointsDevice;  // match_kernels.h
struct MapPointsLock {
  MapPointsLock(orbfe_mappoints* mp);
  ~MapPointsLock();
  MapPointsLock(const MapPointsLock&) = delete;
  MapPointsLock& operator=(const MapPointsLock&) = delete;
  int rc = ORBFE_OK, device = 0;
  const MapPointsDevice* table = nullptr;

 private:
  orbfe_mappoints* held = nullptr;
};

// ---- obsgraph.hip (struct orbfe_obsgraph: obsgraph_handle.h, for the graph's own files only) ----
// How another host file reads a graph's rows on the device, by the route orbfe_obsgraph_update_normal_depth_mappoints takes:
// the constructor takes the handle's serialisation (g == NULL: holds nothing, and table_ready() is a no-op that leaves
// `graph` NULL); the caller then takes its MapPointsLock, and table_ready() writes the marked rows -- complete on return, so
// any stream may read them for the scope.  The capacities and the device are fixed at create.
struct ObsGraphDevice;  // obsgraph_kernels.h
struct ObsGraphLock {
  ObsGraphLock(orbfe_obsgraph* g);
  ~ObsGraphLock();
  ObsGraphLock(const ObsGraphLock&) = delete;
  ObsGraphLock& operator=(const ObsGraphLock&) = delete;
  int table_ready();
  int device = 0, pointCap = 0, kfCap = 0;
  const ObsGraphDevice* graph = nullptr;

 private:
  orbfe_obsgraph* held = nullptr;
};
}  // namespace orbfe

extern "C" {
// ---- extractor_handle.hip (struct orbfe_extractor: extractor_handle.h, for the extractor's own files only) ----
// a consumer of the last extract call's outputs on the handle's own stream: begin orders stream 0 behind every sub-batch
// and returns it, end marks the consumer's last kernel for the next extract call to wait for
int orbfe_extractor_consumer_begin_(orbfe_extractor* e, hipStream_t* s);
int orbfe_extractor_consumer_end_(orbfe_extractor* e);
// how the last extract call was split (S = 0: no call yet); streams / chunkDone: orbfe_extractor::kMaxStreams (32) entries
int orbfe_extractor_split_(orbfe_extractor* e, orbfe::SubSplit* split, hipStream_t* streams, hipEvent_t* chunkDone);
// stage-timer marks for work another translation unit enqueues on a sub-batch stream
void orbfe_extractor_stage_mark_(orbfe_extractor* e, int stage, int sub, int isEnd, hipStream_t s, int frames);
// device pointers of frame `frame` of the handle's own output block (the host-buffer calls)
int orbfe_extractor_output_device_(orbfe_extractor* e, int frame, const orbfe_keypoint** d_kp, const uint8_t** d_desc,
                                   int* n, int* device);
// a frame build that reads the output block was enqueued on `s`: the next call that writes the block waits for it
int orbfe_extractor_reader_end_(orbfe_extractor* e, hipStream_t s);
// stereo_batch.hip: pyramid views + scale tables of the last extract call
int orbfe_stereo_views_(orbfe_extractor* e, int frame, orbfe::PyramidViews* pv, float* scale, float* invScale,
                        int* nlevels, int* device, const float** d_scaleTab);
// extractor_debug.hip: test hooks that hold back / query a stream
int orbfe_debug_stall_launch_(hipStream_t s, int usec);
int orbfe_debug_stream_idle_(hipStream_t s);
// ---- ingest.hip (struct orbfe_rectifier lives there) ----
// the rectification of a sub-batch on that sub-batch's own stream; d_src == NULL only queries w / h / device
int orbfe_remap_launch_(orbfe_rectifier* r, const uint8_t* d_src, int n_frames, int sw, int sh, int sstride,
                        size_t sFrame, uint8_t* d_dst, int dstride, size_t dFrame, hipStream_t stream, int* w, int* h,
                        int* device);
}
