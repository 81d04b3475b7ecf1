// stereo_batch.hip -- host side of the batched stereo matcher on an extractor handle: Frame::ComputeStereoMatches for the
// pairs of the last extract call, the stereo Frame front end in one call, and the pyramid views the matcher files ask for.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "../../include/orbfe.h"
#include "extractor_handle.h"
#include "host_internal.h"
#include "kernels.h"
#include "match_kernels.h"

using namespace orbfe;

// internal (matcher.hip): pyramid views + scale tables of the last extract call
extern "C" int orbfe_stereo_views_(orbfe_extractor* e, int frame, PyramidViews* pv, float* scale, float* invScale,
                                   int* nlevels, int* device, const float** d_scaleTab) {
  if (!e->haveLast) return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: extractor has no pyramid yet");
  int local = 0;
  { int rcf = retained_frame(e, frame, &local); if (rcf) return rcf; }
  HIPCHK(hipSetDevice(e->device));
  { int rcs = sync_all(e); if (rcs) return rcs; }
  *pv = e->lastPyr;
  for (int l = 0; l < pv->nlevels; l++)  // the caller indexes the views with ITS frame number
    pv->lv[l].base -= (size_t)e->lastFrameBase * pv->lv[l].frameStride;
  for (int l = 0; l < e->tab.nlevels; l++) { scale[l] = e->tab.scale[l]; invScale[l] = e->tab.invScale[l]; }
  *nlevels = e->tab.nlevels;
  *device = e->device;
  *d_scaleTab = e->d_scaleTab;
  return ORBFE_OK;
}

// Frame::ComputeStereoMatches for every stereo pair of a device-resident batch (see orbfe.h).
extern "C" int orbfe_stereo_match_batch_device(orbfe_extractor* e, int n_pairs, const orbfe_keypoint* d_keypoints,
                                               const uint8_t* d_descriptors, const int32_t* d_n, int capacity,
                                               float mbf, float mb, float* d_uRight, float* d_depth,
                                               int32_t* d_n_stereo) {
  if (!e || n_pairs < 0 || capacity <= 0 || !d_keypoints || !d_descriptors || !d_n || !d_uRight || !d_depth ||
      !d_n_stereo)
    return fail(ORBFE_ERR_INVALID, "stereo_match_batch_device: bad argument");
  if (n_pairs == 0) return ORBFE_OK;
  if (!e->haveLast || e->last.frames < 2 * n_pairs)
    return fail(ORBFE_ERR_INVALID, "stereo_match_batch_device: the last extract call holds fewer than 2*n_pairs frames");
  if (capacity >= (1 << 20)) return fail(ORBFE_ERR_INVALID, "stereo_match_batch_device: capacity too large");
  HIPCHK(hipSetDevice(e->device));
  const size_t need = (size_t)n_pairs * capacity;
  const int rows = e->lastPyr.lv[0].h;
  const size_t needRows = (size_t)n_pairs * (rows + 1);
  if (need > e->stereoSadCap || needRows > e->stereoRowCap) {
    int rcs = sync_all(e);
    if (rcs) return rcs;
    int rc;
    if ((rc = e->d_stereoSad.alloc(need)) || (rc = e->d_stereoSorted.alloc(need)) || (rc = e->d_stereoRec.alloc(need)) ||
        (rc = e->d_stereoRowStart.alloc(needRows)))
      return rc;
    e->stereoSadCap = need;
    e->stereoRowCap = needRows;
  }
  StereoArgs a = {};
  a.pyrL = e->lastPyr;
  a.pyrR = e->lastPyr;
  a.scaleTab = e->d_scaleTab;
  a.mbf = mbf;
  a.maxD = mbf / mb;  // minZ = mb, maxD = mbf/minZ (src/Frame.cc:542-544)
  if (rows + 1 <= 8192) {  // row index of the right keypoints (k_stereo_bucket)
    a.rowStart = e->d_stereoRowStart;
    a.sortedIdx = e->d_stereoSorted;
    a.sortedRec = e->d_stereoRec;
    a.rows = rows;
    a.bandR = (int)std::ceil(2.0f * e->tab.scale[e->tab.nlevels - 1]) + 2;
  }
  StereoBatch b = {};
  b.kp = reinterpret_cast<const float*>(d_keypoints);
  b.desc = d_descriptors;
  b.n = d_n;
  b.capacity = capacity;
  b.uRight = d_uRight;
  b.depth = d_depth;
  b.sad = e->d_stereoSad;
  // pairs [p0, p0+np) on stream st: every operand moved to the first pair by pointer arithmetic; timed as sub-batch
  // `sub` (< 0: the caller times it)
  auto launch_range = [&](hipStream_t st, int p0, int np, int sub) {
    StereoArgs aa = a;
    StereoBatch bb = b;
    for (int l = 0; l < aa.pyrL.nlevels; l++) {
      aa.pyrL.lv[l].base += (size_t)(2 * p0) * aa.pyrL.lv[l].frameStride;
      aa.pyrR.lv[l].base += (size_t)(2 * p0) * aa.pyrR.lv[l].frameStride;
    }
    if (aa.rowStart) { aa.rowStart += (size_t)p0 * (rows + 1); aa.sortedIdx += (size_t)p0 * capacity; aa.sortedRec += (size_t)p0 * capacity; }
    bb.kp += (size_t)(2 * p0) * capacity * 7;
    bb.desc += (size_t)(2 * p0) * capacity * 32;
    bb.n += 2 * p0;
    bb.uRight += (size_t)p0 * capacity;
    bb.depth += (size_t)p0 * capacity;
    bb.sad += (size_t)p0 * capacity;
    if (knockout_mask(e, false) & 16) return;
    StageTimer t(e, ORBFE_STAGE_MATCH, 1, 2 * np, sub, st);
    launch_stereo_batch(st, aa, bb, np, d_n_stereo + p0);
  };
  const SubSplit& sp = e->last;
  if (!sp.lanes && sp.S > 1 && (sp.per & 1) == 0 && 2 * n_pairs == sp.frames) {
    // The pairs of a sub-batch are matched on that sub-batch's own stream, right behind its extraction: no join of
    // the sub-batch streams, and the (latency-bound) matcher of one sub-batch overlaps the kernels of the others.
    // The next extract call's sub-batch i is enqueued on the same stream, i.e. behind this matcher, by itself.
    int f0, n;
    for (int i = 0; sp.range(i, &f0, &n); i++) {
      launch_range(i == 0 ? e->stream : e->extra[i - 1], f0 / 2, n / 2, i);
      if (i > 0) HIPCHK(hipEventRecord(e->evChunkDone[i], e->extra[i - 1]));  // "sub-batch i done" now includes its matcher
    }
    HIPCHK(hipGetLastError());
    return ORBFE_OK;
  }
  // one launch on stream 0 behind all sub-batches (joined ON THE DEVICE, no host synchronisation)
  { hipStream_t s0; int rc = orbfe_extractor_consumer_begin_(e, &s0); if (rc) return rc; }
  launch_range(e->stream, 0, n_pairs, -1);  // (consumer_begin_/end_ time this form)
  HIPCHK(hipGetLastError());
  // the next extract call's sub-batch streams overwrite the pyramid slabs and the caller's keypoint /
  // descriptor / count buffers this matcher is still reading: they wait for this event (run_pipeline)
  { int rc = orbfe_extractor_consumer_end_(e); if (rc) return rc; }
  return ORBFE_OK;  // asynchronous on the handle's streams: orbfe_extractor_synchronize() to wait
}

// The stereo Frame constructor's front end in ONE call (src/Frame.cc:78-96: ExtractORB on two threads, join,
// ComputeStereoMatches): both eyes go through this handle as a two-frame batch -- one upload, every kernel of the
// single-frame chain over two frames, the stereo matcher on the records that are still in HBM -- and keypoints,
// descriptors, mvuRight and mvDepth come back in one download.  Two handles on two threads + orbfe_compute_stereo_matches
// (which takes the keypoints it has just downloaded up again) cost 0.42-0.51 ms per KITTI pair; this call ~0.3 ms.
extern "C" int orbfe_extract_stereo_frame(orbfe_extractor* e, const uint8_t* left, const uint8_t* right, int width, int height,
                                          int stride, orbfe_keypoint* kpL, uint8_t* descL, int* nL, orbfe_keypoint* kpR,
                                          uint8_t* descR, int* nR, int capacity, float mbf, float mb, float* uRight,
                                          float* depth) {
  if (!e || !nL || !nR) return fail(ORBFE_ERR_INVALID, "extract_stereo_frame: bad argument");
  *nL = *nR = 0;
  if (!left || !right || width <= 0 || height <= 0) return ORBFE_OK;  // empty image: silent return (:1122)
  if (!kpL || !descL || !kpR || !descR || !uRight || !depth || capacity <= 0 || stride < width || capacity >= (1 << 20))
    return fail(ORBFE_ERR_INVALID, "extract_stereo_frame: bad output buffers");
  int rc;
  if ((rc = begin_call(e, width, height, 2, false))) return rc;
  if ((rc = ensure_outputs(e, 2, capacity))) return rc;
  if (e->frameStereoCap < (size_t)capacity) {
    if ((rc = sync_all(e))) return rc;
    e->frameStereoCap = 0;
    if ((rc = e->d_frameStereo.alloc(2 * (size_t)capacity + 16))) return rc;
    e->frameStereoCap = (size_t)capacity;
  }
  // both images into the input slab at the caller's pitch (the kernels read rows in place at any stride)
  const size_t frameStride = ((size_t)stride * height + 255) & ~(size_t)255;
  if ((rc = ensure_host_in(e, 2 * frameStride + 64))) return rc;
  const size_t bytes = (size_t)(height - 1) * stride + width;
  {
    StageTimer t(e, ORBFE_STAGE_H2D, 0, 0, 0, e->stream);
    HIPCHK(hipMemcpyAsync(e->d_hostIn, left, bytes, hipMemcpyHostToDevice, e->stream));
    HIPCHK(hipMemcpyAsync(e->d_hostIn + frameStride, right, bytes, hipMemcpyHostToDevice, e->stream));
  }
  HIPCHK(hipStreamSynchronize(e->stream));  // (as orbfe_extract_batch: sub-batch streams would read the uploaded frames)
  const LevelView l0{e->d_hostIn, frameStride, stride, width, height};
  if ((rc = run_pipeline(e, l0, 2, e->d_kpOut, e->d_descOut, capacity, e->d_nOut))) return rc;
  float* d_ur = e->d_frameStereo;
  float* d_dp = e->d_frameStereo + capacity;
  int32_t* d_ns = reinterpret_cast<int32_t*>(e->d_frameStereo + 2 * (size_t)capacity);
  if ((rc = orbfe_stereo_match_batch_device(e, 1, e->d_kpOut, e->d_descOut, e->d_nOut, capacity, mbf, mb, d_ur, d_dp, d_ns)))
    return rc;
  if (e->last.S > 1 || e->last.lanes) { if ((rc = sync_all(e))) return rc; }  // (a pair is one sub-batch: everything is on e->stream)
  {
    StageTimer t(e, ORBFE_STAGE_D2H, 0, 0, 0, e->stream);
    orbfe_keypoint* kk[2] = {kpL, kpR};
    uint8_t* dd[2] = {descL, descR};
    int n[2] = {0, 0};
    const uint8_t* h_st = nullptr;  // uRight | depth of the left keypoints, `capacity` floats each
    rc = fetch_outputs(e, 2, capacity, kk, dd, n, e->d_frameStereo, 2 * (size_t)capacity * sizeof(float), &h_st);
    if (rc && rc != ORBFE_ERR_CAPACITY) return rc;
    *nL = n[0];
    *nR = n[1];
    if (n[0] > 0) {
      std::memcpy(uRight, h_st, sizeof(float) * (size_t)n[0]);
      std::memcpy(depth, h_st + (size_t)capacity * sizeof(float), sizeof(float) * (size_t)n[0]);
    }
    if (rc) return rc;
  }
  resolve_stage_times(e);
  return ORBFE_OK;
}
