// extractor_debug.hip -- entry points outside the pipeline: single kernels on host buffers, the host-logic debug calls the
// CPU tests compare with the oracle, and the test hook that holds a stream back.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "extractor_handle.h"
#include "host_internal.h"
#include "kernels.h"
#include "octree_host.h"
#include "orb_params.h"

using namespace orbfe;

// ---- standalone primitives on host buffers ----
extern "C" int orbfe_resize_linear(int device, const uint8_t* src, int sw, int sh, int sstride, uint8_t* dst,
                                   int dw, int dh, int dstride) {
  if (!src || !dst || sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || sstride < sw || dstride < dw)
    return fail(ORBFE_ERR_INVALID, "resize: bad argument");
  HIPCHK(hipSetDevice(device));
  ResizeTables t;
  build_resize_tables(sw, sh, dw, dh, &t);
  const int sp = (sw + 63) & ~63, dp = (dw + 63) & ~63;
  DevBuf<uint8_t> d_src, d_dst;
  DevBuf<int32_t> d_xofs, d_yofs;
  DevBuf<int16_t> d_alpha, d_beta;
  DevBuf<uint32_t> d_colrec, d_rowrec;
  int rc;
  if ((rc = d_src.alloc((size_t)sp * sh)) || (rc = d_dst.alloc((size_t)dp * dh))) return rc;
  if ((rc = d_xofs.upload(t.xofs)) || (rc = d_yofs.upload(t.yofs)) || (rc = d_alpha.upload(t.alpha)) || (rc = d_beta.upload(t.beta)))
    return rc;
  if (!t.colrec.empty() && ((rc = d_colrec.upload(t.colrec)) || (rc = d_rowrec.upload(t.rowrec)))) return rc;
  hipError_t err = hipMemcpy2D(d_src, sp, src, sstride, sw, sh, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    launch_resize(nullptr, LevelView{d_src, 0, sp, sw, sh}, LevelViewMut{d_dst, 0, dp, dw, dh}, d_xofs, d_alpha, d_yofs, d_beta,
                  d_colrec, d_rowrec, 1);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy2D(dst, dstride, d_dst, dp, dw, dh, hipMemcpyDeviceToHost);
  if (err != hipSuccess) return fail(ORBFE_ERR_HIP, std::string("resize: ") + hipGetErrorString(err));
  return ORBFE_OK;
}

extern "C" int orbfe_gaussian_blur7(int device, const uint8_t* src, int w, int h, int sstride, uint8_t* dst, int dstride) {
  return orbfe_gaussian_blur7_spec(device, kBlurSpecCv4, src, w, h, sstride, dst, dstride);
}
extern "C" int orbfe_gaussian_blur7_spec(int device, int spec, const uint8_t* src, int w, int h, int sstride, uint8_t* dst, int dstride) {
  if (!src || !dst || w <= 0 || h <= 0 || sstride < w || dstride < w || spec < 0 || spec > 2) return fail(ORBFE_ERR_INVALID, "blur: bad argument");
  HIPCHK(hipSetDevice(device));
  const int p = (w + 63) & ~63;
  DevBuf<uint8_t> d_src, d_dst;
  int rc;
  if ((rc = d_src.alloc((size_t)p * h)) || (rc = d_dst.alloc((size_t)p * h))) return rc;
  hipError_t err = hipMemcpy2D(d_src, p, src, sstride, w, h, hipMemcpyHostToDevice);
  if (err == hipSuccess) {
    launch_blur7(nullptr, LevelView{d_src, 0, p, w, h}, LevelViewMut{d_dst, 0, p, w, h}, 1, spec);
    err = hipGetLastError();
  }
  if (err == hipSuccess) err = hipDeviceSynchronize();
  if (err == hipSuccess) err = hipMemcpy2D(dst, dstride, d_dst, p, w, h, hipMemcpyDeviceToHost);
  if (err != hipSuccess) return fail(ORBFE_ERR_HIP, std::string("blur: ") + hipGetErrorString(err));
  return ORBFE_OK;
}

// Order of the blur kernel's two passes (process-wide, k_blur.hip); the blurred bytes are the same either way.
extern "C" int orbfe_set_blur_pass_order(int order) {
  if (order >= 0) set_blur_pass_order(order);
  return blur_pass_order();
}

// ---- host-logic debug entry points (no GPU needed; CPU tests compare them with the oracle) ----

// DistributeOctTree of the library's host implementation (octree_host.cpp) on flat arrays:
// candidates (x,y relative to minBorder, response) in emission order -> selected (x,y level
// coordinates, response) in list order.  Returns the count or a negative status.
extern "C" int orbfe_debug_octree_host(const uint16_t* xs, const uint16_t* ys, const uint8_t* resp, int n, int minX,
                                       int maxX, int minY, int maxY, int N, uint16_t* out_x, uint16_t* out_y,
                                       uint8_t* out_resp, int cap) {
  if (n < 0 || cap < 0 || (n > 0 && (!xs || !ys || !resp)) || (cap > 0 && (!out_x || !out_y || !out_resp)))
    return fail(ORBFE_ERR_INVALID, "debug_octree_host: bad argument");
  std::vector<Candidate> cand((size_t)(n > 0 ? n : 1));
  for (int i = 0; i < n; i++) { cand[i].xy = (uint32_t)xs[i] | ((uint32_t)ys[i] << 16); cand[i].score = resp[i]; }
  std::vector<LevelKp> out((size_t)(cap > 0 ? cap : 1));
  const int k = distribute_octree_host(cand.data(), n, minX, maxX, minY, maxY, N, out.data(), cap);
  for (int i = 0; i < k && i < cap; i++) { out_x[i] = out[i].x; out_y[i] = out[i].y; out_resp[i] = (uint8_t)out[i].score; }
  return k;
}

// DistributeOctTree of a chosen DEVICE form (k_octree.hip) on n_frames pre-gathered candidate sets of one distribution
// area: one level, the sets are the frames of one launch.  Never runs the host octree.  See include/orbfe.h.
extern "C" int orbfe_debug_octree_device(int device, int form, int n_frames, const uint16_t* xs, const uint16_t* ys,
                                         const uint8_t* resp, const int32_t* n_per_frame, int minX, int maxX, int minY,
                                         int maxY, int N, uint16_t* out_x, uint16_t* out_y, uint16_t* out_resp,
                                         uint16_t* out_rank, int32_t* out_count, int cap, int32_t* info6) {
  const int bw = maxX - minX, bh = maxY - minY;
  if (form < 0 || form > 4 || n_frames < 1 || N < 0 || N > 65532 || minX < 0 || minY < 0 || bw <= 0 || bh <= 0 ||
      maxX > 32767 - kMinBorder || maxY > 32767 - kMinBorder || !info6)
    return fail(ORBFE_ERR_INVALID, "debug_octree_device: bad argument");
  LevelGeom lg;
  std::memset(&lg, 0, sizeof(lg));
  lg.w = bw + 2 * kMinBorder;  // the kernels take the area from the level size and add kMinBorder to what they select
  lg.h = bh + 2 * kMinBorder;
  lg.quota = N;
  octree_level_caps(&lg);
  int maxN = 0;
  size_t total = 0;
  if (n_per_frame)
    for (int f = 0; f < n_frames; f++) {
      if (n_per_frame[f] < 0) return fail(ORBFE_ERR_INVALID, "debug_octree_device: negative candidate count");
      if (n_per_frame[f] > maxN) maxN = n_per_frame[f];
      total += (size_t)n_per_frame[f];
    }
  lg.slotCount = maxN > 0 ? maxN : 1;
  const int maxL = octree_node_capacity(&lg, 1);
  if (maxL <= 0) return fail(ORBFE_ERR_INVALID, "debug_octree_device: set or quota too large for the octree kernels");
  const OctreeForm chosen = octree_choose_form(maxL, n_frames);
  info6[0] = lg.nIni; info6[1] = lg.kpCap; info6[2] = maxL; info6[3] = (int32_t)octree_lds_bytes(maxL);
  info6[4] = (int32_t)kOctreeLdsLimit; info6[5] = (int32_t)chosen;
  if (!out_x) return ORBFE_OK;  // sizes only: no device needed
  if (!n_per_frame || !out_y || !out_resp || !out_rank || !out_count || cap < lg.kpCap || (total > 0 && (!xs || !ys || !resp)))
    return fail(ORBFE_ERR_INVALID, "debug_octree_device: bad buffers (cap must hold kpCap slots per frame)");
  const OctreeForm run = form == 0 ? chosen : (OctreeForm)form;
  if (run != kOctreeGlobal && octree_lds_bytes(maxL) > kOctreeLdsLimit)
    return fail(ORBFE_ERR_INVALID, "debug_octree_device: the node list of this quota does not fit the LDS forms");
  HIPCHK(hipSetDevice(device));
  const size_t F = (size_t)n_frames, slots = (size_t)lg.slotCount, kpCap = (size_t)lg.kpCap;
  std::vector<Candidate> h_cand(F * slots);
  std::memset(h_cand.data(), 0xFF, h_cand.size() * sizeof(Candidate));  // (slots past a frame's count are never read)
  std::vector<int32_t> h_count(F);
  size_t at = 0;
  for (size_t f = 0; f < F; f++) {
    h_count[f] = n_per_frame[f];
    for (int i = 0; i < n_per_frame[f]; i++, at++) {
      h_cand[f * slots + i].xy = (uint32_t)xs[at] | ((uint32_t)ys[at] << 16);
      h_cand[f * slots + i].score = resp[at];
    }
  }
  DevBuf<Candidate> d_cand;
  DevBuf<int32_t> d_candCount, d_levelCount;
  DevBuf<LevelGeom> d_lvg;
  DevBuf<uint16_t> d_nodeOf;
  DevBuf<LevelKp> d_levelKp;
  DevBuf<uint8_t> d_work;
  int rc;
  if ((rc = d_cand.upload(h_cand)) || (rc = d_candCount.upload(h_count)) || (rc = d_lvg.upload(&lg, 1))) return rc;
  if ((rc = d_nodeOf.alloc(F * slots)) || (rc = d_levelKp.alloc(F * kpCap)) || (rc = d_levelCount.alloc(F))) return rc;
  const size_t workStride = run == kOctreeGlobal ? octree_work_stride(maxL) : 0;
  if (workStride && (rc = d_work.alloc(F * workStride))) return rc;
  // every scratch and output array starts as 0xFF bytes: a slot the kernel does not write shows
  HIPCHK(hipMemset(d_nodeOf, 0xFF, F * slots * sizeof(uint16_t)));
  HIPCHK(hipMemset(d_levelKp, 0xFF, F * kpCap * sizeof(LevelKp)));
  HIPCHK(hipMemset(d_levelCount, 0xFF, F * sizeof(int32_t)));
  if (workStride) HIPCHK(hipMemset(d_work, 0xFF, F * workStride));
  OctreeArgs oa = {};
  oa.cand = d_cand;
  oa.slotsPerFrame = lg.slotCount;
  oa.candCount = d_candCount;
  oa.lvg = d_lvg;
  oa.nlevels = 1;
  oa.nodeOf = d_nodeOf;
  oa.levelKp = d_levelKp;
  oa.levelCount = d_levelCount;
  oa.kpSlotsPerFrame = lg.kpCap;
  oa.maxL = maxL;
  oa.narrowLevels = octree_narrow_levels(&lg, 1);
  oa.work = workStride ? d_work.p : nullptr;
  oa.workStride = workStride;
  hipError_t err = launch_octree_form(nullptr, oa, 1, n_frames, run);
  if (err == hipErrorInvalidValue) return fail(ORBFE_ERR_INVALID, "debug_octree_device: the form refused these arguments");
  if (err == hipSuccess) err = hipGetLastError();
  if (err == hipSuccess) err = hipDeviceSynchronize();
  std::vector<LevelKp> h_kp(F * kpCap);
  if (err == hipSuccess) err = hipMemcpy(h_kp.data(), d_levelKp, h_kp.size() * sizeof(LevelKp), hipMemcpyDeviceToHost);
  if (err == hipSuccess) err = hipMemcpy(out_count, d_levelCount, F * sizeof(int32_t), hipMemcpyDeviceToHost);
  if (err != hipSuccess) return fail(ORBFE_ERR_HIP, std::string("debug_octree_device: ") + hipGetErrorString(err));
  for (size_t f = 0; f < F; f++)
    for (size_t i = 0; i < kpCap; i++) {
      const LevelKp k = h_kp[f * kpCap + i];
      const bool written = out_count[f] >= 0 && (int32_t)i < out_count[f];  // the kernel's + kMinBorder becomes + minX / + minY
      out_x[f * cap + i] = written ? (uint16_t)(k.x - kMinBorder + minX) : k.x;
      out_y[f * cap + i] = written ? (uint16_t)(k.y - kMinBorder + minY) : k.y;
      out_resp[f * cap + i] = k.score;
      out_rank[f * cap + i] = k.rank;
    }
  return ORBFE_OK;
}

// The node-array layout of the octree kernels (octree_carve, kernels.h) and the LDS bytes a launch asks for.
extern "C" int orbfe_debug_octree_carve(int maxL, int narrow, int64_t* out11) {
  if (maxL < 4 || maxL > 65532 || (maxL & 3) || !out11) return fail(ORBFE_ERR_INVALID, "debug_octree_carve: bad argument");
  const OctreeCarve c = octree_carve(maxL, narrow ? 2 : 4);
  const uint32_t v[10] = {c.rect0, c.rect1, c.cnt0, c.cnt1, c.child, c.scanA, c.scanB, c.order, c.inS, c.end};
  for (int i = 0; i < 10; i++) out11[i] = v[i];
  out11[10] = (int64_t)octree_lds_bytes(maxL, narrow != 0);
  return ORBFE_OK;
}

// Geometry tables the pipeline derives on the host for a WxH input: per level (w, h, nCols, nRows,
// wCell, hCell, nCells, quota, nIni) as 9 ints, and the FAST grid cells as (level, x0, y0, w, h).
// Returns the number of cells (cells may be NULL to query the count).
extern "C" int orbfe_debug_geometry(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST,
                                    int width, int height, int32_t* levels9, float* tables4, int16_t* cells5,
                                    int cell_cap) {
  if (width <= 0 || height <= 0 || !levels9 || nlevels < 1 || nlevels > ORBFE_MAX_LEVELS)
    return fail(ORBFE_ERR_INVALID, "debug_geometry: bad argument");
  ExtractorTables tab;
  tab.init(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
  if (tables4)
    for (int l = 0; l < tab.nlevels; l++) {
      tables4[l * 4 + 0] = tab.scale[l]; tables4[l * 4 + 1] = tab.invScale[l];
      tables4[l * 4 + 2] = tab.sigma2[l]; tables4[l * 4 + 3] = tab.invSigma2[l];
    }
  FrameGeom g;
  g.build(tab, width, height);
  for (int l = 0; l < g.nlevels; l++) {
    const LevelGeom& v = g.lv[l];
    const int32_t row[9] = {v.w, v.h, v.nCols, v.nRows, v.wCell, v.hCell, v.nCells, v.quota, v.nIni};
    for (int k = 0; k < 9; k++) levels9[l * 9 + k] = row[k];
  }
  if (cells5)
    for (int i = 0; i < g.nFastCells && i < cell_cap; i++) {
      const CellDesc& c = g.cells[i];
      cells5[i * 5 + 0] = c.level; cells5[i * 5 + 1] = c.x0; cells5[i * 5 + 2] = c.y0; cells5[i * 5 + 3] = c.w; cells5[i * 5 + 4] = c.h;
    }
  return g.nFastCells;
}

// Ownership tables of the fused blur + resize kernel (ResizeTables::tileGx / tileDy) with the window start of every
// 4-column group and the upper source row of every output row, for the host-logic test.  n_tiles_x / n_tiles_y come
// back 0 when the fused kernel is not used for this pair of sizes.
extern "C" int orbfe_debug_resize_tiles(int sw, int sh, int dw, int dh, int32_t* tile_gx, int* n_tiles_x, int32_t* tile_dy,
                                        int* n_tiles_y, int32_t* group_start, int32_t* row_upper) {
  if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || !tile_gx || !n_tiles_x || !tile_dy || !n_tiles_y || !group_start || !row_upper)
    return fail(ORBFE_ERR_INVALID, "debug_resize_tiles: bad argument");
  ResizeTables t;
  build_resize_tables(sw, sh, dw, dh, &t);
  *n_tiles_x = *n_tiles_y = 0;
  if (t.tileGx.empty()) return ORBFE_OK;
  *n_tiles_x = (int)t.tileGx.size() - 1;
  *n_tiles_y = (int)t.tileDy.size() - 1;
  std::memcpy(tile_gx, t.tileGx.data(), t.tileGx.size() * 4);   // caller: (sw + 63) / 64 + 1 entries
  std::memcpy(tile_dy, t.tileDy.data(), t.tileDy.size() * 4);   // caller: (sh + 63) / 64 + 1 entries
  const int ngx = (dw + 3) / 4;
  for (int g = 0; g < ngx; g++) group_start[g] = (int32_t)t.colrec[12 * (size_t)g + 8];
  for (int dy = 0; dy < dh; dy++) row_upper[dy] = (int32_t)t.rowrec[4 * (size_t)dy];
  return ORBFE_OK;
}

// cv::resize coefficient tables (xofs, alpha pairs, yofs, beta pairs) the resize kernel uses.
extern "C" int orbfe_debug_resize_tables(int sw, int sh, int dw, int dh, int32_t* xofs, int16_t* alpha, int32_t* yofs,
                                         int16_t* beta) {
  if (sw <= 0 || sh <= 0 || dw <= 0 || dh <= 0 || !xofs || !alpha || !yofs || !beta)
    return fail(ORBFE_ERR_INVALID, "debug_resize_tables: bad argument");
  ResizeTables t;
  build_resize_tables(sw, sh, dw, dh, &t);
  std::memcpy(xofs, t.xofs.data(), t.xofs.size() * 4);
  std::memcpy(alpha, t.alpha.data(), t.alpha.size() * 2);
  std::memcpy(yofs, t.yofs.data(), t.yofs.size() * 4);
  std::memcpy(beta, t.beta.data(), t.beta.size() * 2);
  return ORBFE_OK;
}

// ---- test hook: hold one of the library's streams back (tests/stream_order.py) ----
// One wave; lane 0 polls the 100 MHz constant clock and sleeps between polls.  The kernel writes no memory: whatever
// is enqueued behind it on the same stream simply starts later.  Never used by a product path.
namespace {
__global__ void __launch_bounds__(64) k_debug_stall(long long ticks) {
  if (threadIdx.x != 0) return;
  const long long t0 = (long long)__builtin_amdgcn_s_memrealtime();
  while ((long long)__builtin_amdgcn_s_memrealtime() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}
}  // namespace

// internal (arena.hip): the stall on any stream; usec = 0 is a marker that completes at once
extern "C" int orbfe_debug_stall_launch_(hipStream_t s, int usec) {
  if (usec < 0 || usec > 1000000) return fail(ORBFE_ERR_INVALID, "debug_stall: usec must be 0 .. 1000000");
  hipLaunchKernelGGL(k_debug_stall, dim3(1), dim3(64), 0, s, (long long)usec * 100);
  HIPCHK(hipGetLastError());
  return ORBFE_OK;
}

// internal: 1 when everything enqueued on `s` has completed, 0 while work is pending
extern "C" int orbfe_debug_stream_idle_(hipStream_t s) {
  const hipError_t q = hipStreamQuery(s);
  if (q == hipSuccess) return 1;
  (void)hipGetLastError();  // hipErrorNotReady is the answer, not an error
  if (q == hipErrorNotReady) return 0;
  return fail(ORBFE_ERR_HIP, std::string("debug_stream_idle: ") + hipGetErrorString(q));
}

namespace {
int extractor_stream(orbfe_extractor* e, int stream, hipStream_t* s) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  *s = nullptr;
  if (stream == 0) *s = e->stream;
  else if (stream > 0 && stream < orbfe_extractor::kMaxStreams) *s = e->extra[stream - 1];
  else if (stream == ORBFE_DEBUG_STREAM_H2D) *s = e->sH2D;
  else if (stream == ORBFE_DEBUG_STREAM_D2H) *s = e->sD2H;
  if (!*s) return fail(ORBFE_ERR_INVALID, "debug_stall: the handle has no stream " + std::to_string(stream) + " (yet)");
  HIPCHK(hipSetDevice(e->device));
  return ORBFE_OK;
}
}  // namespace

extern "C" int orbfe_debug_stall_extractor_stream(orbfe_extractor* e, int stream, int usec) {
  hipStream_t s;
  int rc = extractor_stream(e, stream, &s);
  return rc ? rc : orbfe_debug_stall_launch_(s, usec);
}

extern "C" int orbfe_debug_extractor_stream_idle(orbfe_extractor* e, int stream) {
  hipStream_t s;
  int rc = extractor_stream(e, stream, &s);
  return rc ? rc : orbfe_debug_stream_idle_(s);
}
