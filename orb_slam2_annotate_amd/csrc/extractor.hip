// extractor.hip -- the extract calls of include/orbfe.h (replacing ORBextractor::operator(), src/ORBextractor.cc:1119-1197)
// with their host staging, and the reads of what the last call left in the handle.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "extractor_handle.h"
#include "host_internal.h"
#include "kernels.h"
#include "orb_params.h"

using namespace orbfe;

static_assert(sizeof(orbfe_keypoint) == 28, "cv::KeyPoint layout");

// the input slab of the host-buffer calls (frames at the caller's pitch)
int orbfe::ensure_host_in(orbfe_extractor* e, size_t bytes) {
  if (bytes <= e->hostInBytes) return ORBFE_OK;
  // alloc frees the old slab first: until the new one exists nothing may still point at it (the last result's
  // level-0 view lives in it: get_pyramid_level / compute_stereo_matches of the PREVIOUS call would read freed memory)
  e->hostInBytes = 0;
  e->haveLast = false;
  int rc = e->d_hostIn.alloc(bytes);
  if (!rc) e->hostInBytes = bytes;
  return rc;
}
// the pinned staging block of the host-buffer calls: at least 512 KiB, the largest block that comes back in one copy
static int ensure_out_stage(orbfe_extractor* e, size_t bytes) {
  if (bytes <= e->outStageBytes) return ORBFE_OK;
  if (bytes < (size_t)512 * 1024) bytes = (size_t)512 * 1024;
  e->outStageBytes = 0;
  int rc = e->h_outStage.alloc(bytes);
  if (!rc) e->outStageBytes = bytes;
  return rc;
}

// bytes from the start of the output block to the end of the counts of nFrames frames
static size_t out_block_bytes(const orbfe_extractor* e, int nFrames) {
  return (size_t)(reinterpret_cast<uint8_t*>(e->d_nOut) - e->d_outBlock) + sizeof(int32_t) * (size_t)nFrames;
}

// The host-buffer result path: the output block of nFrames frames -- and tailBytes at d_tail behind it -- in ONE copy
// sequence into pinned memory, one synchronisation, then scattered by the CPU: the records of frame f to kps[f] /
// desc[f], its count, clamped to the capacity, to n[f].  The handle then holds the block for
// orbfe_frame_from_extractor.  *h_tail: the staged tail.  ORBFE_ERR_CAPACITY comes after everything is filled.
int orbfe::fetch_outputs(orbfe_extractor* e, int nFrames, int capacity, orbfe_keypoint* const* kps, uint8_t* const* desc, int* n,
                         const void* d_tail, size_t tailBytes, const uint8_t** h_tail) {
  const size_t blockBytes = out_block_bytes(e, nFrames);
  int rc = ensure_out_stage(e, blockBytes + tailBytes);
  if (rc) return rc;
  HIPCHK(hipMemcpyAsync(e->h_outStage, e->d_outBlock, blockBytes, hipMemcpyDeviceToHost, e->stream));
  if (tailBytes) HIPCHK(hipMemcpyAsync(e->h_outStage + blockBytes, d_tail, tailBytes, hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  const uint8_t* hk = e->h_outStage;
  const uint8_t* hd = e->h_outStage + (e->d_descOut - e->d_outBlock);
  const int32_t* hc = reinterpret_cast<const int32_t*>(e->h_outStage + (blockBytes - sizeof(int32_t) * (size_t)nFrames));
  bool overflow = false;
  for (int f = 0; f < nFrames; f++) {
    n[f] = hc[f];
    if (n[f] > capacity) { overflow = true; n[f] = capacity; }
    if (n[f] > 0) {
      std::memcpy(kps[f], hk + (size_t)f * capacity * sizeof(orbfe_keypoint), sizeof(orbfe_keypoint) * (size_t)n[f]);
      std::memcpy(desc[f], hd + (size_t)f * capacity * 32, (size_t)n[f] * 32);
    }
  }
  if (h_tail) *h_tail = e->h_outStage + blockBytes;
  e->outLastCount.assign(n, n + nFrames);
  e->outLastCapacity = capacity;
  e->outLastFrames = nFrames;
  return overflow ? fail(ORBFE_ERR_CAPACITY, "keypoint capacity too small") : ORBFE_OK;
}

extern "C" int orbfe_extract_batch_device_async(orbfe_extractor* e, const uint8_t* d_images, int n_frames,
                                                int width, int height, int stride, size_t frame_stride,
                                                orbfe_keypoint* d_keypoints, uint8_t* d_descriptors,
                                                int capacity, int32_t* d_n_out) {
  if (!e || !d_keypoints || !d_descriptors || !d_n_out || capacity <= 0 || n_frames < 0)
    return fail(ORBFE_ERR_INVALID, "extract_batch_device: bad argument");
  if (n_frames == 0) return ORBFE_OK;
  if (!d_images || width <= 0 || height <= 0 || stride < width)
    return fail(ORBFE_ERR_INVALID, "extract_batch_device: bad image");
  if (frame_stride < (size_t)stride * (size_t)height)  // rows are staged up to the PITCH (16-byte requests): see orbfe.h
    return fail(ORBFE_ERR_INVALID, "extract_batch_device: frame_stride < stride * height (every frame must be readable for stride * height bytes)");
  int rc = begin_call(e, width, height, n_frames, false);  // (the outputs are the caller's)
  if (rc) return rc;
  LevelView l0{d_images, frame_stride, stride, width, height};
  return run_pipeline(e, l0, n_frames, d_keypoints, d_descriptors, capacity, d_n_out);
}

// Examples/Stereo/stereo_euroc.cc:136-137 (cv::remap of the left and of the right image) in front of the two ExtractORB
// calls of the stereo Frame constructor (src/Frame.cc:78-81), for a device-resident batch of raw pairs: sub-batch by
// sub-batch, on the sub-batch's own stream -- rectified frames are written interleaved (L0, R0, L1, R1, ...), the layout
// orbfe_stereo_match_batch_device reads.
namespace {
struct RectifyCtx {
  orbfe_rectifier *rl, *rr;
  const uint8_t *rawL, *rawR;
  int sw, sh, sstride;
  size_t sFrame;
  uint8_t* rect;
  int w, h;
};
int rectify_chunk(void* c, hipStream_t s, int f0, int n) {
  const RectifyCtx* x = static_cast<const RectifyCtx*>(c);
  if ((f0 & 1) || (n & 1)) return fail(ORBFE_ERR_INVALID, "extract_stereo_rectified: a sub-batch splits a stereo pair");
  const size_t fr = (size_t)x->w * x->h;
  const int p0 = f0 / 2, np = n / 2;
  int rc = orbfe_remap_launch_(x->rl, x->rawL + (size_t)p0 * x->sFrame, np, x->sw, x->sh, x->sstride, x->sFrame,
                               x->rect + (size_t)f0 * fr, x->w, 2 * fr, s, nullptr, nullptr, nullptr);
  if (rc) return rc;
  return orbfe_remap_launch_(x->rr, x->rawR + (size_t)p0 * x->sFrame, np, x->sw, x->sh, x->sstride, x->sFrame,
                             x->rect + (size_t)(f0 + 1) * fr, x->w, 2 * fr, s, nullptr, nullptr, nullptr);
}
}  // namespace

extern "C" int orbfe_extract_stereo_rectified_batch_device_async(
    orbfe_extractor* e, orbfe_rectifier* rect_left, orbfe_rectifier* rect_right, const uint8_t* d_raw_left,
    const uint8_t* d_raw_right, int n_pairs, int src_width, int src_height, int src_stride, size_t src_frame_stride,
    uint8_t* d_rectified, orbfe_keypoint* d_keypoints, uint8_t* d_descriptors, int capacity, int32_t* d_n_out) {
  if (!e || !rect_left || !rect_right || !d_keypoints || !d_descriptors || !d_n_out || capacity <= 0 || n_pairs < 0)
    return fail(ORBFE_ERR_INVALID, "extract_stereo_rectified: bad argument");
  if (n_pairs == 0) return ORBFE_OK;
  if (!d_raw_left || !d_raw_right || !d_rectified || src_width <= 0 || src_height <= 0 || src_stride < src_width ||
      src_frame_stride < (size_t)src_stride * (src_height - 1) + src_width)
    return fail(ORBFE_ERR_INVALID, "extract_stereo_rectified: bad image");
  int wl, hl, dl, wr, hr, dr, rc;
  if ((rc = orbfe_remap_launch_(rect_left, nullptr, 0, 0, 0, 0, 0, nullptr, 0, 0, nullptr, &wl, &hl, &dl))) return rc;
  if ((rc = orbfe_remap_launch_(rect_right, nullptr, 0, 0, 0, 0, 0, nullptr, 0, 0, nullptr, &wr, &hr, &dr))) return rc;
  if (wl != wr || hl != hr || dl != e->device || dr != e->device)
    return fail(ORBFE_ERR_INVALID, "extract_stereo_rectified: the two rectifiers differ in size or device from each other / the extractor");
  const int n_frames = 2 * n_pairs;
  if ((rc = begin_call(e, wl, hl, n_frames, false))) return rc;  // (as orbfe_extract_batch_device_async: the outputs are the caller's)
  RectifyCtx ctx{rect_left, rect_right, d_raw_left, d_raw_right, src_width, src_height, src_stride, src_frame_stride,
                 d_rectified, wl, hl};
  PreChunk pre;
  pre.fn = rectify_chunk;
  pre.ctx = &ctx;
  LevelView l0{d_rectified, (size_t)wl * hl, wl, wl, hl};
  return run_pipeline(e, l0, n_frames, d_keypoints, d_descriptors, capacity, d_n_out, nullptr, 0, &pre);
}

extern "C" int orbfe_extract_batch_device(orbfe_extractor* e, const uint8_t* d_images, int n_frames,
                                          int width, int height, int stride, size_t frame_stride,
                                          orbfe_keypoint* d_keypoints, uint8_t* d_descriptors,
                                          int capacity, int32_t* d_n_out) {
  int rc = orbfe_extract_batch_device_async(e, d_images, n_frames, width, height, stride, frame_stride,
                                            d_keypoints, d_descriptors, capacity, d_n_out);
  if (rc) return rc;
  return orbfe_extractor_synchronize(e);
}

extern "C" int orbfe_extract_batch(orbfe_extractor* e, const uint8_t* images, int n_frames, int width,
                                   int height, int stride, size_t frame_stride,
                                   orbfe_keypoint* keypoints, uint8_t* descriptors, int capacity,
                                   int* n_out) {
  if (!e || !n_out || n_frames < 0) return fail(ORBFE_ERR_INVALID, "extract_batch: bad argument");
  for (int f = 0; f < n_frames; f++) n_out[f] = 0;
  if (n_frames == 0) return ORBFE_OK;
  if (!images || width <= 0 || height <= 0) return ORBFE_OK;  // empty image: silent return (:1122)
  if (!keypoints || !descriptors || capacity <= 0 || stride < width)
    return fail(ORBFE_ERR_INVALID, "extract_batch: bad output buffers");
  bool pinnedIn = false;
  {
    hipPointerAttribute_t at;
    pinnedIn = hipPointerGetAttributes(&at, images) == hipSuccess && at.type != hipMemoryTypeUnregistered;
    (void)hipGetLastError();
  }
  if (!e->hostOctree && frame_stride >= (size_t)stride * (height - 1) + width && (pinnedIn ? n_frames >= 32 : n_frames >= 512))
    // a real batch: chunked H2D / kernels / D2H overlapped on separate streams instead of upload-all, compute,
    // download-all.  Pageable buffers would have to be page-locked for the call, which costs milliseconds (measured
    // 5-9 ms for 128 VGA frames) and only pays for very large batches; pinned ones (orbfe_host_alloc) always pay.
    return orbfe_extract_batch_pipelined(e, images, n_frames, width, height, stride, frame_stride, keypoints, descriptors,
                                         capacity, n_out, 0);
  int rc;
  if ((rc = begin_call(e, width, height, n_frames, true))) return rc;  // an earlier asynchronous call may still use the workspace
  if ((rc = ensure_outputs(e, n_frames, capacity))) return rc;
  const FrameGeom& g = e->geom;
  LevelView l0{e->d_pyr + g.lv[0].off, g.pyrBytes, g.lv[0].pitch, width, height};
  const bool tight = frame_stride == (size_t)stride * height || n_frames == 1;
  {
    StageTimer t(e, ORBFE_STAGE_H2D, 0, 0, 0, e->stream);
    if (tight && stride != g.lv[0].pitch) {
      // ONE linear copy of the frames as they lie in host memory into an input slab of the caller's pitch, which the
      // kernels read in place at any stride (like caller-owned device frames).  A 2-D copy of rows that are not a
      // multiple of the DMA granule degenerates into one descriptor per row: 3.0 ms for ONE 1241 x 376 frame (0.15 GB/s)
      // against 0.1 ms this way -- the live-camera latency of a KITTI frame was that copy.
      const size_t bytes = (size_t)(n_frames - 1) * frame_stride + (size_t)(height - 1) * stride + width;
      // the slab is readable for stride * height bytes per frame: the kernels stage rows up to the pitch, not the width
      if ((rc = ensure_host_in(e, (size_t)(n_frames - 1) * frame_stride + (size_t)stride * height + 64))) return rc;
      HIPCHK(hipMemcpyAsync(e->d_hostIn, images, bytes, hipMemcpyHostToDevice, e->stream));
      l0 = LevelView{e->d_hostIn, frame_stride, stride, width, height};
    } else {
      // level 0 lives at the head of the per-frame pyramid slab (pitch-aligned copy)
      for (int f = 0; f < n_frames; f++)
        HIPCHK(hipMemcpy2DAsync(e->d_pyr + (size_t)f * g.pyrBytes + g.lv[0].off, g.lv[0].pitch,
                                images + (size_t)f * frame_stride, stride, width, height,
                                hipMemcpyHostToDevice, e->stream));
    }
  }
  // (the sub-batch streams read the uploaded frames.  Round 4 measured a single frame -- everything on e->stream, in order --
  // without this wait and without the one behind the kernels: 0.206 / 0.168 ms per KITTI / VGA frame against 0.205 / 0.158
  // with them, same box, three alternations: the waits are not what a frame's 60 us outside its kernels is made of)
  HIPCHK(hipStreamSynchronize(e->stream));
  if ((rc = run_pipeline(e, l0, n_frames, e->d_kpOut, e->d_descOut, capacity, e->d_nOut))) return rc;
  if ((rc = sync_all(e))) return rc;
  {
    StageTimer t(e, ORBFE_STAGE_D2H, 0, 0, 0, e->stream);
    if (out_block_bytes(e, n_frames) <= (size_t)512 * 1024) {
      // small batch (the live-camera case): everything in ONE copy into pinned memory, then scattered
      // by the CPU -- one DMA + one synchronisation instead of 1 + 2*n_frames copies and two syncs
      std::vector<orbfe_keypoint*> kk(n_frames);
      std::vector<uint8_t*> dd(n_frames);
      for (int f = 0; f < n_frames; f++) { kk[f] = keypoints + (size_t)f * capacity; dd[f] = descriptors + (size_t)f * capacity * 32; }
      if ((rc = fetch_outputs(e, n_frames, capacity, kk.data(), dd.data(), n_out))) {
        e->outLastFrames = 0;  // (an overflowing batch leaves no block to build frames from)
        return rc;
      }
    } else {
      bool overflow = false;
      std::vector<int32_t> cnt(n_frames);
      HIPCHK(hipMemcpyAsync(cnt.data(), e->d_nOut, sizeof(int32_t) * n_frames, hipMemcpyDeviceToHost, e->stream));
      HIPCHK(hipStreamSynchronize(e->stream));
      for (int f = 0; f < n_frames; f++) {
        int n = cnt[f];
        if (n > capacity) { overflow = true; n = capacity; }
        n_out[f] = n;
        if (n > 0) {
          HIPCHK(hipMemcpyAsync(keypoints + (size_t)f * capacity, e->d_kpOut + (size_t)f * capacity,
                                sizeof(orbfe_keypoint) * n, hipMemcpyDeviceToHost, e->stream));
          HIPCHK(hipMemcpyAsync(descriptors + (size_t)f * capacity * 32, e->d_descOut + (size_t)f * capacity * 32,
                                (size_t)n * 32, hipMemcpyDeviceToHost, e->stream));
        }
      }
      HIPCHK(hipStreamSynchronize(e->stream));
      if (overflow) return fail(ORBFE_ERR_CAPACITY, "keypoint capacity too small");
      e->outLastCount.assign(n_out, n_out + n_frames);
      e->outLastCapacity = capacity;
      e->outLastFrames = n_frames;
    }
  }
  resolve_stage_times(e);
  return ORBFE_OK;
}

// ---- the pipelined host-batch path (end-to-end form of operator()) ----
namespace {
// page-locks [p, p+bytes) for the duration of a call when the caller did not allocate it with orbfe_host_alloc
struct ScopedPin {
  void* p = nullptr;
  int pin(const void* ptr, size_t bytes) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, ptr) == hipSuccess && at.type != hipMemoryTypeUnregistered) return ORBFE_OK;  // already pinned
    (void)hipGetLastError();
    if (hipHostRegister(const_cast<void*>(ptr), bytes, hipHostRegisterDefault) != hipSuccess) {
      (void)hipGetLastError();
      return ORBFE_OK;  // pageable memory still works (the runtime stages it), only slower
    }
    p = const_cast<void*>(ptr);
    return ORBFE_OK;
  }
  ~ScopedPin() { if (p) (void)hipHostUnregister(p); }
};
}  // namespace

// ORBextractor::operator() for a host batch, end to end: images in host memory -> keypoints and descriptors in host
// memory (src/ORBextractor.cc:1119-1197 per frame).  The batch is cut into chunks; the H2D copy of chunk k+1, the
// kernels of chunk k and the D2H copy of chunk k-1 run at the same time on three sets of streams (two input slabs and
// two output blocks in HBM, ordered by events; no host wait inside the loop).  Outputs use the layout of
// orbfe_extract_batch: frame f at keypoints + f*capacity, descriptors + f*capacity*32; rows past n_out[f] are
// unspecified.  Host buffers from orbfe_host_alloc (pinned) transfer at PCIe speed; others are page-locked for the
// duration of the call.
extern "C" int orbfe_extract_batch_pipelined(orbfe_extractor* e, const uint8_t* images, int n_frames, int width, int height,
                                             int stride, size_t frame_stride, orbfe_keypoint* keypoints,
                                             uint8_t* descriptors, int capacity, int* n_out, int chunk_frames) {
  if (!e || !n_out || n_frames < 0) return fail(ORBFE_ERR_INVALID, "extract_batch_pipelined: bad argument");
  for (int f = 0; f < n_frames; f++) n_out[f] = 0;
  if (n_frames == 0) return ORBFE_OK;
  if (!images || width <= 0 || height <= 0) return ORBFE_OK;  // empty image: silent return (:1122)
  if (!keypoints || !descriptors || capacity <= 0 || stride < width || frame_stride < (size_t)stride * (height - 1) + width)
    return fail(ORBFE_ERR_INVALID, "extract_batch_pipelined: bad buffers");
  int C = chunk_frames > 0 ? chunk_frames : 256;
  if (C > n_frames) C = n_frames;
  int rc = begin_call(e, width, height, C, true);  // (as orbfe_extract_batch_device_async: the outputs are the caller's)
  if (rc) return rc;
  if (!e->sH2D) {
    HIPCHK(stream_get(e->device, kRoleH2D, &e->sH2D));
    HIPCHK(stream_get(e->device, kRoleD2H, &e->sD2H));
    for (int i = 0; i < 2; i++) {
      HIPCHK(hipEventCreateWithFlags(&e->evIn[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&e->evComp[i], hipEventDisableTiming));
      HIPCHK(hipEventCreateWithFlags(&e->evOutDone[i], hipEventDisableTiming));
    }
  }
  // device input slab: tightly packed host frames are uploaded as they are (ONE linear copy per chunk, row pitch =
  // the caller's stride, which the kernels read in place whatever its alignment; only $ORBFE_COPY_UNALIGNED=1 repacks
  // an odd pitch in run_chunk) -- a 2-D copy of 1241-byte rows
  // degenerates into one DMA descriptor per row and ran at 0.1 GB/s; only batches with gaps between the frames
  // take the per-frame 2-D form into a 64-byte pitch
  const bool tight = frame_stride == (size_t)stride * height;
  const int pitch = tight ? stride : (width + 63) & ~63;
  const size_t inBytes = (size_t)C * pitch * height;
  const size_t kpB = ((size_t)C * capacity * sizeof(orbfe_keypoint) + 255) & ~(size_t)255;
  const size_t deB = ((size_t)C * capacity * 32 + 255) & ~(size_t)255;
  const size_t outBytes = kpB + deB + (size_t)C * 4;
  if (inBytes > e->pipeInBytes || outBytes > e->pipeOutBytes) {
    HIPCHK(hipStreamSynchronize(e->sH2D));
    HIPCHK(hipStreamSynchronize(e->sD2H));
    for (int i = 0; i < 2; i++) {
      if ((rc = e->d_pipeIn[i].alloc(inBytes))) return rc;
      if ((rc = e->d_pipeOut[i].alloc(outBytes))) return rc;
    }
    e->pipeInBytes = inBytes;
    e->pipeOutBytes = outBytes;
  }
  ScopedPin pinIn, pinKp, pinDesc;
  pinIn.pin(images, frame_stride * (size_t)(n_frames - 1) + (size_t)stride * (height - 1) + width);
  pinKp.pin(keypoints, (size_t)n_frames * capacity * sizeof(orbfe_keypoint));
  pinDesc.pin(descriptors, (size_t)n_frames * capacity * 32);
  PinBuf<int32_t> h_cnt;  // counts come back through a small pinned block of their own
  if ((rc = h_cnt.alloc((size_t)n_frames))) return rc;
  const int nChunks = (n_frames + C - 1) / C;
  int status = ORBFE_OK;
  for (int k = 0; k < nChunks && status == ORBFE_OK; k++) {
    const int slot = k & 1;
    const int f0 = k * C, n = f0 + C <= n_frames ? C : n_frames - f0;
    auto H = [&](hipError_t err) { if (err != hipSuccess && status == ORBFE_OK) status = fail(ORBFE_ERR_HIP, hipGetErrorString(err)); };
    // input slab `slot` is free once the kernels of chunk k-2 are done
    if (k >= 2) H(hipStreamWaitEvent(e->sH2D, e->evComp[slot], 0));
    if (tight) {
      // (up to the last pixel of the chunk's last frame: the caller's array may end there)
      H(hipMemcpyAsync(e->d_pipeIn[slot], images + (size_t)f0 * frame_stride,
                       (size_t)(n - 1) * frame_stride + (size_t)(height - 1) * stride + width, hipMemcpyHostToDevice, e->sH2D));
    } else {
      for (int f = 0; f < n; f++)
        H(hipMemcpy2DAsync(e->d_pipeIn[slot] + (size_t)f * pitch * height, pitch, images + (size_t)(f0 + f) * frame_stride, stride,
                           width, height, hipMemcpyHostToDevice, e->sH2D));
    }
    H(hipEventRecord(e->evIn[slot], e->sH2D));
    // kernels: wait for the upload, and for the D2H of chunk k-2 before its output block is overwritten
    hipEvent_t waits[2] = {e->evIn[slot], e->evOutDone[slot]};
    orbfe_keypoint* d_kp = reinterpret_cast<orbfe_keypoint*>(e->d_pipeOut[slot].p);
    uint8_t* d_de = e->d_pipeOut[slot] + kpB;
    int32_t* d_n = reinterpret_cast<int32_t*>(e->d_pipeOut[slot] + kpB + deB);
    if (k > 0) next_event_slot(e);  // (chunk 0 records into the call's own slot)
    LevelView l0{e->d_pipeIn[slot], (size_t)pitch * height, pitch, width, height};
    if (status == ORBFE_OK) {
      rc = run_pipeline(e, l0, n, d_kp, d_de, capacity, d_n, waits, k >= 2 ? 2 : 1);
      if (rc) { status = rc; break; }
      e->lastFrameBase = f0;  // the pyramid / blurred levels / candidates that stay behind are those of frames [f0, f0 + n)
    }
    for (int i = 1; i < e->chunksPending; i++) H(hipStreamWaitEvent(e->stream, e->evChunkDone[i], 0));  // join the sub-batches
    H(hipEventRecord(e->evComp[slot], e->stream));
    // results of this chunk straight into the caller's arrays
    H(hipStreamWaitEvent(e->sD2H, e->evComp[slot], 0));
    H(hipMemcpyAsync(keypoints + (size_t)f0 * capacity, d_kp, (size_t)n * capacity * sizeof(orbfe_keypoint), hipMemcpyDeviceToHost, e->sD2H));
    H(hipMemcpyAsync(descriptors + (size_t)f0 * capacity * 32, d_de, (size_t)n * capacity * 32, hipMemcpyDeviceToHost, e->sD2H));
    H(hipMemcpyAsync(h_cnt + f0, d_n, sizeof(int32_t) * (size_t)n, hipMemcpyDeviceToHost, e->sD2H));
    H(hipEventRecord(e->evOutDone[slot], e->sD2H));
  }
  hipError_t e1 = hipStreamSynchronize(e->sD2H);
  int rc2 = sync_all(e);
  hipError_t e2 = hipStreamSynchronize(e->sH2D);
  bool overflow = false;
  if (status == ORBFE_OK && e1 == hipSuccess && e2 == hipSuccess && rc2 == ORBFE_OK)
    for (int f = 0; f < n_frames; f++) {
      int n = h_cnt[f];
      if (n > capacity) { overflow = true; n = capacity; }
      n_out[f] = n;
    }
  resolve_stage_times(e);
  if (status != ORBFE_OK) return status;
  if (e1 != hipSuccess) return fail(ORBFE_ERR_HIP, hipGetErrorString(e1));
  if (e2 != hipSuccess) return fail(ORBFE_ERR_HIP, hipGetErrorString(e2));
  if (rc2) return rc2;
  if (overflow) return fail(ORBFE_ERR_CAPACITY, "keypoint capacity too small");
  return ORBFE_OK;
}

extern "C" int orbfe_extract(orbfe_extractor* e, const uint8_t* image, int width, int height, int stride,
                             orbfe_keypoint* keypoints, uint8_t* descriptors, int capacity, int* n_out) {
  return orbfe_extract_batch(e, image, 1, width, height, stride, (size_t)stride * (size_t)(height > 0 ? height : 0),
                             keypoints, descriptors, capacity, n_out);
}

// frame index of the LAST extract call -> index into what the handle still holds.  The chunked (pipelined) host path keeps
// the intermediate data of its last chunk only: frames before it fail loudly instead of silently answering with another
// frame's pyramid.
int orbfe::retained_frame(orbfe_extractor* e, int frame, int* local) {
  if (!e->haveLast) return fail(ORBFE_ERR_INVALID, "no extract call yet");
  const int f = frame - e->lastFrameBase;
  if (frame < 0 || f >= e->last.frames) return fail(ORBFE_ERR_INVALID, "frame out of range");
  if (f < 0)
    return fail(ORBFE_ERR_INVALID, "pyramid of frame " + std::to_string(frame) + " not retained: the pipelined host path keeps the last chunk only (frames " +
                                       std::to_string(e->lastFrameBase) + ".." + std::to_string(e->lastFrameBase + e->last.frames - 1) + ")");
  *local = f;
  return ORBFE_OK;
}

static int copy_level_out(orbfe_extractor* e, const PyramidViews& pv, int frame, int level, uint8_t* dst, int dst_stride) {
  if (!e || !dst) return fail(ORBFE_ERR_INVALID, "NULL argument");
  { int rcf = retained_frame(e, frame, &frame); if (rcf) return rcf; }
  if (level < 0 || level >= pv.nlevels)
    return fail(ORBFE_ERR_INVALID, "frame/level out of range");
  const LevelView& v = pv.lv[level];
  if (dst_stride < v.w) return fail(ORBFE_ERR_INVALID, "dst_stride too small");
  HIPCHK(hipSetDevice(e->device));
  { int rcs = sync_all(e); if (rcs) return rcs; }
  HIPCHK(hipMemcpy2DAsync(dst, dst_stride, v.base + (size_t)frame * v.frameStride, v.pitch, v.w, v.h,
                          hipMemcpyDeviceToHost, e->stream));
  HIPCHK(hipStreamSynchronize(e->stream));
  return ORBFE_OK;
}
extern "C" int orbfe_extractor_get_pyramid_level(orbfe_extractor* e, int frame, int level, uint8_t* dst, int dst_stride) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  return copy_level_out(e, e->lastPyr, frame, level, dst, dst_stride);
}
extern "C" int orbfe_extractor_debug_blurred_level(orbfe_extractor* e, int frame, int level, uint8_t* dst, int dst_stride) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  return copy_level_out(e, e->lastBlur, frame, level, dst, dst_stride);
}
extern "C" int orbfe_extractor_pyramid_level_device(orbfe_extractor* e, int frame, int level, const uint8_t** d_ptr,
                                                    int* pitch, int* w, int* h) {
  if (!e || !d_ptr || !pitch || !w || !h) return fail(ORBFE_ERR_INVALID, "NULL argument");
  { int rcf = retained_frame(e, frame, &frame); if (rcf) return rcf; }
  if (level < 0 || level >= e->lastPyr.nlevels) return fail(ORBFE_ERR_INVALID, "frame/level out of range");
  const LevelView& v = e->lastPyr.lv[level];
  *d_ptr = v.base + (size_t)frame * v.frameStride;
  *pitch = v.pitch;
  *w = v.w;
  *h = v.h;
  return ORBFE_OK;
}

extern "C" int orbfe_extractor_debug_candidates(orbfe_extractor* e, int frame, int level, float* xs, float* ys,
                                                float* resp, int cap) {
  if (!e || !xs || !ys || !resp) return fail(ORBFE_ERR_INVALID, "NULL argument");
  { int rcf = retained_frame(e, frame, &frame); if (rcf) return rcf; }
  if (level < 0 || level >= e->geom.nlevels) return fail(ORBFE_ERR_INVALID, "frame/level out of range");
  HIPCHK(hipSetDevice(e->device));
  { int rcs = sync_all(e); if (rcs) return rcs; }
  int32_t n = 0;
  HIPCHK(hipMemcpy(&n, e->d_candCount + (size_t)frame * e->geom.nlevels + level, 4, hipMemcpyDeviceToHost));
  std::vector<Candidate> c((size_t)(n > 0 ? n : 1));
  if (n > 0)
    HIPCHK(hipMemcpy(c.data(), e->d_cand + (size_t)frame * e->geom.totalSlots + e->geom.lv[level].slotStart,
                     sizeof(Candidate) * n, hipMemcpyDeviceToHost));
  for (int i = 0; i < n && i < cap; i++) {
    xs[i] = (float)(c[i].xy & 0xffffu);
    ys[i] = (float)(c[i].xy >> 16);
    resp[i] = (float)c[i].score;
  }
  return n;
}
