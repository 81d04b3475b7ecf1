// frames.hip -- C-ABI entry points of the resident Frame / KeyFrame handle (include/orbfe.h: orbfe_frame_*; frame.h): the
// three builds, orbfe_frame_set_featvec, synchronise and release, and the list of frames a call has yet to settle.  A build
// is one staged copy into the frame's slab and the grid build on the calling thread's stream, with no host wait.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "frame.h"
#include "host_internal.h"
#include "kernels.h"
#include "match_kernels.h"

using namespace orbfe;

namespace orbfe {
bool featvec_ok(const orbfe_featvec* f, int n) {
  if (!f || f->n_nodes < 0) return false;
  if (f->n_nodes == 0) return true;
  if (!f->node_ids || !f->offsets || !f->indices) return false;
  if (f->offsets[0] != 0) return false;
  for (int i = 0; i < f->n_nodes; i++) {
    if (f->offsets[i + 1] < f->offsets[i]) return false;
    if (i > 0 && f->node_ids[i] <= f->node_ids[i - 1]) return false;
  }
  const int tot = f->offsets[f->n_nodes];
  for (int i = 0; i < tot; i++)
    if (f->indices[i] >= (uint32_t)n) return false;
  return true;
}

namespace {
thread_local std::vector<const orbfe_frame*> t_unsettled;
}  // namespace
hipError_t frame_use(Arena* ar, const orbfe_frame* f) {
  if (!f || f->settled.load(std::memory_order_acquire)) return hipSuccess;
  hipError_t e = hipStreamWaitEvent(ar->stream, f->ready, 0);
  if (e == hipSuccess) t_unsettled.push_back(f);
  return e;
}
void frames_settle() {  // call after the stream of the call has been synchronised
  for (const orbfe_frame* f : t_unsettled) f->settled.store(true, std::memory_order_release);
  t_unsettled.clear();
}
UnsettledScope::UnsettledScope() { t_unsettled.clear(); }
UnsettledScope::~UnsettledScope() { t_unsettled.clear(); }
}  // namespace orbfe

extern "C" void orbfe_frame_release(orbfe_frame* f) {
  if (!f) return;
  (void)hipSetDevice(f->device);
  // a frame whose own upload may still be in flight (released before any search used it): its slab must not be handed
  // to the next upload until then
  if (f->ready && !f->settled.load(std::memory_order_acquire)) (void)hipEventSynchronize(f->ready);
  for (size_t i = 0; i < t_unsettled.size();)
    if (t_unsettled[i] == f) t_unsettled.erase(t_unsettled.begin() + (long)i); else i++;
  slab_put(&f->slab);
  event_put(f->device, f->ready);
  delete f;
}

extern "C" const orbfe_frame_view* orbfe_frame_get_view(const orbfe_frame* f) { return f ? &f->view : nullptr; }

namespace {
// host side of a resident frame: copies of what the claim loops / gates read, the canonical view, the slab layout
struct FrameLayout { size_t oX, oY, oA, oU, oO, oK, oC, oI, oD, oS, total; };
int frame_host_init(const char* who, int device, const orbfe_frame_view* v, const orbfe_featvec* fv, orbfe_frame** outF,
                    FrameLayout* L, size_t* nIdxOut) {
  if (!v || v->n < 0 || v->n > GRID_MAX_FEATURES || !(v->max_x > v->min_x) || !(v->max_y > v->min_y) ||
      (v->n > 0 && (!v->x || !v->y || !v->octave || !v->desc)))
    return fail(ORBFE_ERR_INVALID, std::string(who) + ": bad frame view (x, y, octave, desc and the image bounds are required)");
  const int n = v->n;
  if (fv && !featvec_ok(fv, n)) return fail(ORBFE_ERR_INVALID, std::string(who) + ": malformed FeatureVector");
  orbfe_frame* f = new (std::nothrow) orbfe_frame();
  if (!f) return fail(ORBFE_ERR_NOMEM, "out of memory");
  f->device = device; f->n = n;
  f->hx.assign(v->x, v->x + n); f->hy.assign(v->y, v->y + n); f->hoct.assign(v->octave, v->octave + n);
  f->hdesc.assign(v->desc, v->desc + (size_t)n * 32);
  if (v->angle) f->hangle.assign(v->angle, v->angle + n);
  if (v->u_right) f->hur.assign(v->u_right, v->u_right + n);
  f->hstereo.assign((size_t)n, 0);
  if (v->u_right) for (int i = 0; i < n; i++) f->hstereo[i] = v->u_right[i] >= 0 ? 1 : 0;
  size_t nIdx = 0;
  if (fv) {
    f->haveFv = true;
    if (fv->n_nodes > 0) {  // (an EMPTY FeatureVector may come with NULL arrays: nothing is read from them)
      f->nodeIds.assign(fv->node_ids, fv->node_ids + fv->n_nodes);
      f->offsets.assign(fv->offsets, fv->offsets + fv->n_nodes + 1);
      nIdx = (size_t)fv->offsets[fv->n_nodes];
      f->hindices.assign(fv->indices, fv->indices + nIdx);
    } else {
      f->offsets.assign(1, 0);
    }
    f->fv.n_nodes = fv->n_nodes; f->fv.node_ids = f->nodeIds.data(); f->fv.offsets = f->offsets.data(); f->fv.indices = f->hindices.data();
  }
  orbfe_frame_view& c = f->view;
  c.n = n; c.x = f->hx.data(); c.y = f->hy.data(); c.octave = f->hoct.data();
  c.angle = v->angle ? f->hangle.data() : nullptr;
  c.u_right = v->u_right ? f->hur.data() : nullptr;
  c.desc = f->hdesc.data();
  c.min_x = v->min_x; c.max_x = v->max_x; c.min_y = v->min_y; c.max_y = v->max_y;
  c.resident = f;
  // one slab: x y angle u_right | octave | key | cell | indices | desc | stereo.  The index list gets room for one index per
  // feature even when no FeatureVector comes with the upload: orbfe_frame_set_featvec may attach it later (Frame::ComputeBoW
  // runs after the constructor, src/Tracking.cc:836-843)
  const size_t N = (size_t)(n ? n : 1);
  size_t off = 0;
  auto place = [&](size_t bytes) { const size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
  // what always comes from the host first (mvuRight, stereo flags, index list, then the positions), what the device can
  // supply behind it (angles, octaves, descriptors), what the grid build writes last: an upload is ONE copy of [0, oK), a
  // frame built from the extractor's records ONE copy of [0, oX) (or [0, oA) with caller-undistorted positions)
  L->oU = place(N * 4); L->oS = place(N); L->oI = place((nIdx > N ? nIdx : N) * 4); L->oX = place(N * 4); L->oY = place(N * 4);
  L->oA = place(N * 4); L->oO = place(N * 4); L->oD = place(N * 32); L->oK = place(N * 4); L->oC = place(3073 * 4);
  L->total = off;
  hipError_t err = hipSetDevice(device);
  if (err == hipSuccess) err = slab_get(device, off, &f->slab);
  if (err == hipSuccess) err = event_get(device, &f->ready);
  if (err != hipSuccess) {
    orbfe_frame_release(f);
    return fail(hip_status(err), std::string(who) + ": " + hipGetErrorString(err));
  }
  f->settled.store(false);
  uint8_t* b = (uint8_t*)f->slab.p;
  f->dx = (float*)(b + L->oX); f->dy = (float*)(b + L->oY); f->dangle = (float*)(b + L->oA); f->dur = (float*)(b + L->oU);
  f->doct = (int32_t*)(b + L->oO); f->dkey = (uint32_t*)(b + L->oK); f->dcell = (int32_t*)(b + L->oC); f->dindices = (uint32_t*)(b + L->oI);
  f->ddesc = b + L->oD; f->dstereo = b + L->oS;
  *outF = f;
  *nIdxOut = nIdx;
  return ORBFE_OK;
}

// grid build behind whatever filled the slab, then the ready event: NO host wait (frame_use orders the consumers)
hipError_t frame_finish(Arena* ar, orbfe_frame* f, const orbfe_frame_view* v) {
  GridFrame g{};
  g.x = f->dx; g.y = f->dy; g.octave = f->doct; g.uRight = v->u_right ? f->dur : nullptr; g.desc = f->ddesc; g.n = f->n;
  g.minX = v->min_x; g.minY = v->min_y;
  g.wInv = 64.0f / (v->max_x - v->min_x);
  g.hInv = 48.0f / (v->max_y - v->min_y);
  launch_grid_build(ar->stream, g, f->dkey, f->dcell);
  hipError_t err = hipGetLastError();
  if (err == hipSuccess) err = hipEventRecord(f->ready, ar->stream);
  return err;
}
}  // namespace

extern "C" int orbfe_frame_upload(int device, const orbfe_frame_view* v, const orbfe_featvec* fv, orbfe_frame** out) {
  if (!out) return fail(ORBFE_ERR_INVALID, "frame_upload: NULL argument");
  *out = nullptr;
  orbfe_frame* f = nullptr;
  FrameLayout L;
  size_t nIdx = 0;
  int rc = frame_host_init("frame_upload", device, v, fv, &f, &L, &nIdx);
  if (rc != ORBFE_OK) return rc;
  const int n = f->n;
  // only what the searches read goes up: the key / cell arrays behind it are written by the grid build
  const size_t upBytes = L.oK;
  Arena* ar;
  // staged through the thread's pinned mirror: one copy up, then the grid build (Frame::AssignFeaturesToGrid, once)
  hipError_t err = arena_stream(device, &ar);
  if (err == hipSuccess) err = staging_reserve(upBytes);
  if (err == hipSuccess) {
    uint8_t* h = thread_staging().h;
    if (n) {
      std::memcpy(h + L.oX, f->hx.data(), (size_t)n * 4); std::memcpy(h + L.oY, f->hy.data(), (size_t)n * 4);
      if (v->angle) std::memcpy(h + L.oA, f->hangle.data(), (size_t)n * 4); else std::memset(h + L.oA, 0, (size_t)n * 4);
      if (v->u_right) std::memcpy(h + L.oU, f->hur.data(), (size_t)n * 4); else std::memset(h + L.oU, 0, (size_t)n * 4);
      std::memcpy(h + L.oO, f->hoct.data(), (size_t)n * 4);
      std::memcpy(h + L.oD, f->hdesc.data(), (size_t)n * 32);
      std::memcpy(h + L.oS, f->hstereo.data(), (size_t)n);
    }
    if (nIdx) std::memcpy(h + L.oI, f->hindices.data(), nIdx * 4);
    // ONE copy (every further hipMemcpyAsync costs the host ~5 us)
    err = hipMemcpyAsync(f->slab.p, h, upBytes, hipMemcpyHostToDevice, ar->stream);
    if (err == hipSuccess) err = staging_mark_pending(ar->stream);  // the next use of the staging buffer waits for these copies
  }
  if (err == hipSuccess) err = frame_finish(ar, f, v);
  if (err != hipSuccess) { orbfe_frame_release(f); return fail(hip_status(err), std::string("frame_upload: ") + hipGetErrorString(err)); }
  *out = f;
  return ORBFE_OK;
}

// Frame::Frame (src/Frame.cc:61-117) is extract -> undistort -> stereo -> grid: the keypoint records and descriptors the
// extractor produced are still in HBM when the Frame is built.  orbfe_frame_from_device makes the resident operands from
// THOSE (28-byte records -> x / y / angle / octave arrays, descriptors device to device, grid built on the device): of
// the frame's 60 bytes per keypoint only mvuRight (and, with ORBFE_FRAME_XY_FROM_VIEW, the undistorted positions) travel
// over PCIe.  `view` holds the host arrays the claim loops read (what orbfe_extract returned to the caller, after its own
// UndistortKeyPoints); view->n records are taken.
extern "C" int orbfe_frame_from_device(int device, const orbfe_keypoint* d_keypoints, const uint8_t* d_descriptors,
                                       const orbfe_frame_view* view, const orbfe_featvec* fv, int flags, orbfe_frame** out) {
  if (!out) return fail(ORBFE_ERR_INVALID, "frame_from_device: NULL argument");
  *out = nullptr;
  if (view && view->n > 0 && (!d_keypoints || !d_descriptors)) return fail(ORBFE_ERR_INVALID, "frame_from_device: NULL device arrays");
  orbfe_frame* f = nullptr;
  FrameLayout L;
  size_t nIdx = 0;
  int rc = frame_host_init("frame_from_device", device, view, fv, &f, &L, &nIdx);
  if (rc != ORBFE_OK) return rc;
  const int n = f->n;
  const bool xyFromView = (flags & ORBFE_FRAME_XY_FROM_VIEW) != 0;
  Arena* ar;
  hipError_t err = arena_stream(device, &ar);
  // host part: mvuRight + stereo flags + the FeatureVector's index list (+ positions), adjacent at the head of the slab:
  // ONE copy through the pinned staging
  const size_t hostBytes = xyFromView ? L.oA : L.oX;
  const bool anyHost = view->u_right || nIdx || xyFromView;
  if (err == hipSuccess && anyHost) err = staging_reserve(hostBytes);
  if (err == hipSuccess && n && anyHost) {
    uint8_t* h = thread_staging().h;
    if (view->u_right) { std::memcpy(h + L.oU, f->hur.data(), (size_t)n * 4); std::memcpy(h + L.oS, f->hstereo.data(), (size_t)n); }
    else { std::memset(h + L.oU, 0, (size_t)n * 4); std::memset(h + L.oS, 0, (size_t)n); }
    if (nIdx) std::memcpy(h + L.oI, f->hindices.data(), nIdx * 4);
    if (xyFromView) { std::memcpy(h + L.oX, f->hx.data(), (size_t)n * 4); std::memcpy(h + L.oY, f->hy.data(), (size_t)n * 4); }
    err = hipMemcpyAsync(f->slab.p, h, hostBytes, hipMemcpyHostToDevice, ar->stream);
    if (err == hipSuccess) err = staging_mark_pending(ar->stream);
  }
  if (err == hipSuccess && n) {
    launch_frame_from_records(ar->stream, reinterpret_cast<const float*>(d_keypoints), d_descriptors, n, xyFromView ? nullptr : f->dx,
                              xyFromView ? nullptr : f->dy, f->dangle, f->doct, f->ddesc, anyHost ? nullptr : f->dstereo);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = frame_finish(ar, f, view);
  if (err != hipSuccess) { orbfe_frame_release(f); return fail(hip_status(err), std::string("frame_from_device: ") + hipGetErrorString(err)); }
  *out = f;
  return ORBFE_OK;
}

extern "C" int orbfe_frame_from_extractor(orbfe_extractor* e, int frame, const orbfe_frame_view* view, const orbfe_featvec* fv,
                                          int flags, orbfe_frame** out) {
  if (!out) return fail(ORBFE_ERR_INVALID, "frame_from_extractor: NULL argument");
  *out = nullptr;
  const orbfe_keypoint* dkp = nullptr;
  const uint8_t* ddesc = nullptr;
  int n = 0, device = 0;
  int rc = orbfe_extractor_output_device_(e, frame, &dkp, &ddesc, &n, &device);
  if (rc != ORBFE_OK) return rc;
  if (!view || view->n > n) return fail(ORBFE_ERR_INVALID, "frame_from_extractor: the view holds more keypoints than the extractor produced for this frame");
  rc = orbfe_frame_from_device(device, dkp, ddesc, view, fv, flags, out);
  if (rc != ORBFE_OK) return rc;
  // the build reads the handle's output block on this thread's stream without a host wait: the handle's next call that
  // rewrites the block waits for it
  Arena* ar;
  hipError_t err = arena_stream(device, &ar);
  rc = err == hipSuccess ? orbfe_extractor_reader_end_(e, ar->stream)
                         : fail(hip_status(err), std::string("frame_from_extractor: ") + hipGetErrorString(err));
  if (rc != ORBFE_OK) { orbfe_frame_release(*out); *out = nullptr; }
  return rc;
}

// Frame::ComputeBoW runs after the constructor (src/Tracking.cc:836-843, src/Frame.cc:433-440): attach the FeatureVector
// to a frame that was made resident without one.  Call it before any search uses the frame (it rewrites the index list);
// the calling thread may differ from the building one (LocalMapping's KeyFrame::ComputeBoW): frame_use orders the copy.
extern "C" int orbfe_frame_set_featvec(orbfe_frame* f, const orbfe_featvec* fv) {
  UnsettledScope unsettledScope;
  if (!f || !fv) return fail(ORBFE_ERR_INVALID, "frame_set_featvec: NULL argument");
  if (!featvec_ok(fv, f->n)) return fail(ORBFE_ERR_INVALID, "frame_set_featvec: malformed FeatureVector");
  const size_t nIdx = fv->n_nodes > 0 ? (size_t)fv->offsets[fv->n_nodes] : 0;
  if (nIdx > (size_t)(f->n ? f->n : 1)) return fail(ORBFE_ERR_INVALID, "frame_set_featvec: more indices than features");
  if (fv->n_nodes > 0) {
    f->nodeIds.assign(fv->node_ids, fv->node_ids + fv->n_nodes);
    f->offsets.assign(fv->offsets, fv->offsets + fv->n_nodes + 1);
    f->hindices.assign(fv->indices, fv->indices + nIdx);
  } else {
    f->nodeIds.clear(); f->hindices.clear(); f->offsets.assign(1, 0);
  }
  f->fv.n_nodes = fv->n_nodes; f->fv.node_ids = f->nodeIds.data(); f->fv.offsets = f->offsets.data(); f->fv.indices = f->hindices.data();
  f->haveFv = true;
  if (nIdx == 0) return ORBFE_OK;
  Arena* ar;
  hipError_t err = arena_stream(f->device, &ar);
  if (err == hipSuccess) err = staging_reserve(nIdx * 4);
  // the frame's own build copy covers the index region and may still be queued on the building thread's stream
  if (err == hipSuccess) err = frame_use(ar, f);
  if (err == hipSuccess) {
    uint8_t* h = thread_staging().h;
    std::memcpy(h, f->hindices.data(), nIdx * 4);
    err = hipMemcpyAsync(f->dindices, h, nIdx * 4, hipMemcpyHostToDevice, ar->stream);
  }
  if (err == hipSuccess) err = hipStreamSynchronize(ar->stream);  // (the handle may be in use on other streams afterwards)
  if (err != hipSuccess) return fail(hip_status(err), std::string("frame_set_featvec: ") + hipGetErrorString(err));
  frames_settle();
  return ORBFE_OK;
}

extern "C" int orbfe_frame_synchronize(const orbfe_frame* f) {
  if (!f) return fail(ORBFE_ERR_INVALID, "frame_synchronize: NULL frame");
  if (f->settled.load(std::memory_order_acquire)) return ORBFE_OK;
  hipError_t err = hipSetDevice(f->device);
  if (err == hipSuccess) err = hipEventSynchronize(f->ready);
  if (err != hipSuccess) return fail(hip_status(err), std::string("frame_synchronize: ") + hipGetErrorString(err));
  f->settled.store(true, std::memory_order_release);
  return ORBFE_OK;
}
