// ingest.hip -- C-ABI entry points of the steps next to the hot path (include/orbfe.h, "Next to the path"): colour -> gray,
// MapPoint::ComputeDistinctiveDescriptors, the EuRoC rectification (cv::initUndistortRectifyMap, cv::remap) behind the
// orbfe_rectifier handle, cv::undistortPoints and Frame::ComputeStereoFromRGBD.  The kernels are k_ingest.hip.
//   a host-array call     stages through the calling thread's arena: one copy up, the launch on the thread's matcher stream, one
//                         copy back, complete on return.  A strided float image is packed row by row into the arena's mirror;
//                         the 8-bit images of orbfe_cvt_gray / orbfe_remap go between the caller's rows and the arena directly
//                         (image_up / image_down).  Either way the caller's padding beyond a row's width is neither read nor
//                         written.
//   a device-pointer call (*_batch_device) is enqueued on the default stream -- the library knows no stream for arrays the
//                         caller wrote, and the default stream is what orders the kernel behind the caller's default-stream
//                         work -- and waits for that stream alone: complete on return.
#include <hip/hip_runtime.h>

#include <cstring>
#include <memory>
#include <string>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "ingest_kernels.h"

using namespace orbfe;

// The float maps are converted once, at create time, to what cv::remap converts them to for every tile of every frame
// (k_remap_convert, k_ingest.hip).
struct orbfe_rectifier {
  int device = 0;
  int width = 0, height = 0;  // destination size = map size
  DevBuf<uint32_t> xy;        // [height][pitch]
  DevBuf<uint16_t> phase;     // [height][pitch]
  int pitch = 0;              // multiple of 4
};

namespace {

const hipStream_t kDefaultStream = nullptr;  // (the device-pointer calls)

// `rows` rows of `rowBytes` bytes each, the rows `srcStride` / `dstStride` bytes apart
void copy_rows(void* dst, size_t dstStride, const void* src, size_t srcStride, size_t rowBytes, int rows) {
  if (dstStride == rowBytes && srcStride == rowBytes) {
    std::memcpy(dst, src, rowBytes * (size_t)rows);
    return;
  }
  for (int y = 0; y < rows; y++)
    std::memcpy(static_cast<uint8_t*>(dst) + (size_t)y * dstStride, static_cast<const uint8_t*>(src) + (size_t)y * srcStride, rowBytes);
}
// rows in: a host image of `stride` elements per row, packed to `width` elements per row in the mirror
template <typename T>
hipError_t up_rows(Arena* a, T** d, const T* h, int width, int height, int stride) {
  return up_pack(a, d, (size_t)width * height, [&](T* m) {
    copy_rows(m, (size_t)width * sizeof(T), h, (size_t)stride * sizeof(T), (size_t)width * sizeof(T), height);
  });
}
// A whole 8-bit image in and a whole one out (orbfe_cvt_gray, orbfe_remap) travel between the caller's rows and the arena
// directly, on the arena's stream: through the mirror each would be copied a second time on the host, which for 0.3 .. 0.9 MB
// costs more than the one staged copy saves (profiles/ingest_arena_latency.txt).  `width` bytes of each row, as above.
hipError_t image_up(Arena* a, uint8_t* d, const uint8_t* h, int width, int height, int stride) {
  return hipMemcpy2DAsync(d, (size_t)width, h, (size_t)stride, (size_t)width, (size_t)height, hipMemcpyHostToDevice, a->stream);
}
hipError_t image_down(Arena* a, uint8_t* h, int stride, const uint8_t* d, int pitch, int width, int height) {
  return hipMemcpy2DAsync(h, (size_t)stride, d, (size_t)pitch, (size_t)width, (size_t)height, hipMemcpyDeviceToHost, a->stream);
}

int remap_launch(orbfe_rectifier* r, const uint8_t* d_src, int n_frames, int sw, int sh, int sstride, size_t sFrame,
                 uint8_t* d_dst, int dstride, size_t dFrame, hipStream_t stream) {
  launch_remap(stream, r->xy.p, r->phase.p, r->pitch, r->width, r->height, n_frames, d_src, sw, sh, sstride, sFrame, d_dst, dstride,
               dFrame);
  HIPCHK(hipGetLastError());
  return ORBFE_OK;
}

bool undistort_params(const float* K4, const float* dist, int n_dist, UndistortParams* p) {
  if (!K4 || n_dist < 0 || n_dist > 8 || (n_dist > 0 && !dist) || !(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8))
    return false;
  p->fx = (double)K4[0]; p->fy = (double)K4[1]; p->cx = (double)K4[2]; p->cy = (double)K4[3];
  p->ifx = 1. / p->fx; p->ify = 1. / p->fy;
  for (int i = 0; i < 8; i++) p->k[i] = i < n_dist ? (double)dist[i] : 0.0;
  p->iters = n_dist > 0 ? 5 : 1;
  return true;
}

}  // namespace

extern "C" int orbfe_cvt_gray(int device, const uint8_t* src, int width, int height, int stride, int channels,
                              int rgb_order, uint8_t* dst, int dst_stride) {
  if (!src || !dst || width <= 0 || height <= 0 || (channels != 3 && channels != 4) || stride < width * channels ||
      dst_stride < width)
    return fail(ORBFE_ERR_INVALID, "cvt_gray: bad argument");
  uint8_t *ds, *dd;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    ds = carve<uint8_t>(a, (size_t)width * channels * height);
    dd = carve<uint8_t>(a, (size_t)width * height);
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(image_up(ar, ds, src, width * channels, height, stride));
  launch_cvt_gray(ar->stream, ds, width, height, width * channels, 0, channels, rgb_order, dd, width, 0, 1);
  HIPCHK(hipGetLastError());
  HIPCHK(image_down(ar, dst, dst_stride, dd, width, width, height));
  HIPCHK(hipStreamSynchronize(ar->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_cvt_gray_batch_device(int device, const uint8_t* d_src, int n_frames, int width, int height,
                                           int stride, size_t frame_stride, int channels, int rgb_order,
                                           uint8_t* d_dst, int dst_stride, size_t dst_frame_stride) {
  if (!d_src || !d_dst || n_frames < 0 || width <= 0 || height <= 0 || (channels != 3 && channels != 4) ||
      stride < width * channels || dst_stride < width)
    return fail(ORBFE_ERR_INVALID, "cvt_gray_batch_device: bad argument");
  if (n_frames == 0) return ORBFE_OK;
  HIPCHK(hipSetDevice(device));
  launch_cvt_gray(kDefaultStream, d_src, width, height, stride, frame_stride, channels, rgb_order, d_dst, dst_stride,
                  dst_frame_stride, n_frames);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(kDefaultStream));
  return ORBFE_OK;
}

extern "C" int orbfe_distinctive_descriptors(int device, const uint8_t* descriptors, const int32_t* offsets,
                                             int n_points, int32_t* best_index) {
  if (n_points < 0 || (n_points > 0 && (!descriptors || !offsets || !best_index)))
    return fail(ORBFE_ERR_INVALID, "distinctive_descriptors: bad argument");
  if (n_points == 0) return ORBFE_OK;
  for (int i = 0; i < n_points; i++)
    if (offsets[i + 1] < offsets[i] || offsets[i + 1] - offsets[i] > 65535)
      return fail(ORBFE_ERR_INVALID, "distinctive_descriptors: bad offsets (or more than 65535 observations)");
  if (offsets[0] != 0) return fail(ORBFE_ERR_INVALID, "distinctive_descriptors: offsets[0] != 0");
  const size_t total = (size_t)offsets[n_points];
  uint8_t* dd;
  int32_t *doff, *dbest;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dd, descriptors, total * 32));
    TRY(up(a, &doff, offsets, (size_t)n_points + 1));
    open_span(a);
    dbest = carve<int32_t>(a, (size_t)n_points);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_distinctive(ar->stream, dd, doff, n_points, dbest);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(best_index, mirror_of(ar, dbest), (size_t)n_points * 4);
  return ORBFE_OK;
}

// internal (extractor.hip): the rectification of a sub-batch enqueued on that sub-batch's own stream
extern "C" int orbfe_remap_launch_(orbfe_rectifier* r, const uint8_t* d_src, int n_frames, int sw, int sh, int sstride,
                                   size_t sFrame, uint8_t* d_dst, int dstride, size_t dFrame, hipStream_t stream, int* w, int* h,
                                   int* device) {
  if (!r) return fail(ORBFE_ERR_INVALID, "NULL rectifier");
  if (w) *w = r->width;
  if (h) *h = r->height;
  if (device) *device = r->device;
  if (!d_src || n_frames <= 0) return ORBFE_OK;  // query only
  return remap_launch(r, d_src, n_frames, sw, sh, sstride, sFrame, d_dst, dstride, dFrame, stream);
}

extern "C" int orbfe_rectifier_create(int device, const float* map_x, const float* map_y, int width, int height,
                                  int map_stride, orbfe_rectifier** out) {
  if (!map_x || !map_y || !out || width <= 0 || height <= 0 || map_stride < width || width > 32767 || height > 32767)
    return fail(ORBFE_ERR_INVALID, "remap_create: bad argument");
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<orbfe_rectifier> r(new orbfe_rectifier());
  r->device = device; r->width = width; r->height = height; r->pitch = (width + 3) & ~3;
  const size_t n = (size_t)r->pitch * height;
  int rc;
  if ((rc = r->xy.alloc(n)) || (rc = r->phase.alloc(n))) return rc;
  float *dmx, *dmy;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up_rows(a, &dmx, map_x, width, height, map_stride));
    return up_rows(a, &dmy, map_y, width, height, map_stride);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_remap_convert(ar->stream, dmx, dmy, width, width, height, r->pitch, r->xy.p, r->phase.p);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ar->stream));  // (the handle's two arrays are the outputs: nothing comes back)
  *out = r.release();
  return ORBFE_OK;
}

extern "C" void orbfe_rectifier_destroy(orbfe_rectifier* r) {
  if (!r) return;
  (void)hipSetDevice(r->device);
  delete r;
}

extern "C" int orbfe_remap(orbfe_rectifier* r, const uint8_t* src, int src_width, int src_height, int src_stride,
                           uint8_t* dst, int dst_stride) {
  if (!r || !src || !dst || src_width <= 0 || src_height <= 0 || src_stride < src_width || dst_stride < r->width)
    return fail(ORBFE_ERR_INVALID, "remap: bad argument");
  uint8_t *ds, *dd;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    ds = carve<uint8_t>(a, (size_t)src_width * src_height);
    dd = carve<uint8_t>(a, (size_t)r->pitch * r->height);
    return hipSuccess;
  };
  HIPCHK(arena_stage(r->device, &ar, stage));
  HIPCHK(image_up(ar, ds, src, src_width, src_height, src_stride));
  int rc;
  if ((rc = remap_launch(r, ds, 1, src_width, src_height, src_width, 0, dd, r->pitch, 0, ar->stream))) return rc;
  HIPCHK(image_down(ar, dst, dst_stride, dd, r->pitch, r->width, r->height));
  HIPCHK(hipStreamSynchronize(ar->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_remap_batch_device(orbfe_rectifier* r, const uint8_t* d_src, int n_frames, int src_width,
                                        int src_height, int src_stride, size_t src_frame_stride, uint8_t* d_dst,
                                        int dst_stride, size_t dst_frame_stride) {
  if (!r || !d_src || !d_dst || n_frames < 0 || src_width <= 0 || src_height <= 0 || src_stride < src_width ||
      dst_stride < r->width)
    return fail(ORBFE_ERR_INVALID, "remap_batch_device: bad argument");
  if (n_frames == 0) return ORBFE_OK;
  HIPCHK(hipSetDevice(r->device));
  const int rc = remap_launch(r, d_src, n_frames, src_width, src_height, src_stride, src_frame_stride, d_dst, dst_stride,
                              dst_frame_stride, kDefaultStream);
  if (rc != ORBFE_OK) return rc;
  HIPCHK(hipStreamSynchronize(kDefaultStream));
  return ORBFE_OK;
}

// cv::initUndistortRectifyMap(K, D, R, P[:3,:3], size, CV_32F, M1, M2) as Examples/Stereo/stereo_euroc.cc:97-98 calls it,
// once at start-up: the two float maps orbfe_rectifier_create takes (k_init_rectify_map, k_ingest.hip).
extern "C" int orbfe_init_undistort_rectify_map(int device, const double* K, const double* D, int n_dist, const double* R,
                                                const double* P, int width, int height, float* map_x, float* map_y) {
  if (!K || width <= 0 || height <= 0 || !map_x || !map_y || !(n_dist == 0 || n_dist == 4 || n_dist == 5 || n_dist == 8) ||
      (n_dist > 0 && !D))
    return fail(ORBFE_ERR_INVALID, "init_undistort_rectify_map: bad argument (K, the maps and 0 / 4 / 5 / 8 distortion coefficients are required)");
  static const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const double *Rm = R ? R : I3, *Ar = P ? P : K;
  // iR = (P * R)^-1: nine dot products and cv::invert's closed 3 x 3 form -- a dozen double operations of set-up, evaluated
  // here in the order the reference evaluates them (host: this translation unit is built with -ffp-contract=off)
  double M[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      double acc = 0;
      for (int k = 0; k < 3; k++) acc += Ar[3 * i + k] * Rm[3 * k + j];
      M[3 * i + j] = acc;
    }
  double d = M[0] * (M[4] * M[8] - M[5] * M[7]) - M[1] * (M[3] * M[8] - M[5] * M[6]) + M[2] * (M[3] * M[7] - M[4] * M[6]);
  if (d == 0) return fail(ORBFE_ERR_INVALID, "init_undistort_rectify_map: P * R is singular");
  d = 1. / d;
  RectifyMapParams p;
  p.ir[0] = (M[4] * M[8] - M[5] * M[7]) * d; p.ir[1] = (M[2] * M[7] - M[1] * M[8]) * d; p.ir[2] = (M[1] * M[5] - M[2] * M[4]) * d;
  p.ir[3] = (M[5] * M[6] - M[3] * M[8]) * d; p.ir[4] = (M[0] * M[8] - M[2] * M[6]) * d; p.ir[5] = (M[2] * M[3] - M[0] * M[5]) * d;
  p.ir[6] = (M[3] * M[7] - M[4] * M[6]) * d; p.ir[7] = (M[1] * M[6] - M[0] * M[7]) * d; p.ir[8] = (M[0] * M[4] - M[1] * M[3]) * d;
  p.fx = K[0]; p.fy = K[4]; p.u0 = K[2]; p.v0 = K[5];
  p.k1 = n_dist > 0 ? D[0] : 0; p.k2 = n_dist > 1 ? D[1] : 0; p.p1 = n_dist > 2 ? D[2] : 0; p.p2 = n_dist > 3 ? D[3] : 0;
  p.k3 = n_dist >= 5 ? D[4] : 0; p.k4 = n_dist >= 8 ? D[5] : 0; p.k5 = n_dist >= 8 ? D[6] : 0; p.k6 = n_dist >= 8 ? D[7] : 0;
  p.w = width; p.h = height;
  const size_t n = (size_t)width * height;
  float *dmx, *dmy;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    open_span(a);
    dmx = carve<float>(a, n);
    dmy = carve<float>(a, n);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_init_rectify_map(ar->stream, p, dmx, dmy);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(map_x, mirror_of(ar, dmx), n * 4);
  std::memcpy(map_y, mirror_of(ar, dmy), n * 4);
  return ORBFE_OK;
}

extern "C" int orbfe_undistort_points(int device, const float* xy, int n, const float* K4, const float* dist,
                                      int n_dist, float* out_xy) {
  UndistortParams p;
  if (n < 0 || (n > 0 && (!xy || !out_xy)) || !undistort_params(K4, dist, n_dist, &p))
    return fail(ORBFE_ERR_INVALID, "undistort_points: bad argument");
  if (n == 0) return ORBFE_OK;
  float *din, *dout;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &din, xy, (size_t)n * 2));
    open_span(a);
    dout = carve<float>(a, (size_t)n * 2);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_undistort_points(ar->stream, p, din, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(out_xy, mirror_of(ar, dout), (size_t)n * 8);
  return ORBFE_OK;
}

extern "C" int orbfe_undistort_keypoints_batch_device(int device, const orbfe_keypoint* d_keypoints,
                                                      const int32_t* d_n, int n_frames, int capacity,
                                                      const float* K4, const float* dist, int n_dist,
                                                      orbfe_keypoint* d_keypoints_un) {
  UndistortParams p;
  if (!d_keypoints || !d_n || !d_keypoints_un || n_frames < 0 || capacity <= 0 || !undistort_params(K4, dist, n_dist, &p))
    return fail(ORBFE_ERR_INVALID, "undistort_keypoints_batch_device: bad argument");
  if (n_frames == 0) return ORBFE_OK;
  HIPCHK(hipSetDevice(device));
  launch_undistort_keypoints(kDefaultStream, p, reinterpret_cast<const float*>(d_keypoints), d_n, capacity, n_frames,
                             reinterpret_cast<float*>(d_keypoints_un));
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(kDefaultStream));
  return ORBFE_OK;
}

extern "C" int orbfe_compute_image_bounds(int device, int cols, int rows, const float* K4, const float* dist,
                                          int n_dist, float* bounds4) {
  if (!bounds4 || cols <= 0 || rows <= 0) return fail(ORBFE_ERR_INVALID, "compute_image_bounds: bad argument");
  if (n_dist > 0 && dist && dist[0] != 0.0) {
    const float in[8] = {0.0f, 0.0f, (float)cols, 0.0f, 0.0f, (float)rows, (float)cols, (float)rows};
    float out[8];
    const int rc = orbfe_undistort_points(device, in, 4, K4, dist, n_dist, out);
    if (rc != ORBFE_OK) return rc;
    bounds4[0] = out[4] < out[0] ? out[4] : out[0];  // min(mat(0,0), mat(2,0)), src/Frame.cc:496-499
    bounds4[1] = out[2] < out[6] ? out[6] : out[2];
    bounds4[2] = out[3] < out[1] ? out[3] : out[1];
    bounds4[3] = out[5] < out[7] ? out[7] : out[5];
  } else {
    bounds4[0] = 0.0f; bounds4[1] = (float)cols; bounds4[2] = 0.0f; bounds4[3] = (float)rows;
  }
  return ORBFE_OK;
}

extern "C" int orbfe_stereo_from_rgbd(int device, const float* kx, const float* ky, const float* kux, int n,
                                      const float* depth_image, int width, int height, int stride_floats, float mbf,
                                      float* u_right, float* depth) {
  if (n < 0 || width <= 0 || height <= 0 || stride_floats < width || !depth_image ||
      (n > 0 && (!kx || !ky || !kux || !u_right || !depth)))
    return fail(ORBFE_ERR_INVALID, "stereo_from_rgbd: bad argument");
  for (int i = 0; i < n; i++)
    if (!(kx[i] >= 0 && ky[i] >= 0 && (int)kx[i] < width && (int)ky[i] < height))
      return fail(ORBFE_ERR_INVALID, "stereo_from_rgbd: keypoint outside the depth image");
  if (n == 0) return ORBFE_OK;
  float *dimg, *dkx, *dky, *dkux, *dur, *ddp;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up_rows(a, &dimg, depth_image, width, height, stride_floats));
    TRY(up(a, &dkx, kx, (size_t)n));
    TRY(up(a, &dky, ky, (size_t)n));
    TRY(up(a, &dkux, kux, (size_t)n));
    open_span(a);
    dur = carve<float>(a, (size_t)n);
    ddp = carve<float>(a, (size_t)n);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_stereo_from_rgbd(ar->stream, dkx, dky, dkux, n, dimg, width, mbf, dur, ddp);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(u_right, mirror_of(ar, dur), (size_t)n * 4);
  std::memcpy(depth, mirror_of(ar, ddp), (size_t)n * 4);
  return ORBFE_OK;
}
