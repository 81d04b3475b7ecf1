// ingest_kernels.h -- argument blocks and launchers of the ingest kernels (k_ingest.hip; host side: ingest.hip).  A launcher
// holds the grid arithmetic of its kernel and enqueues it on `s`; the caller reads hipGetLastError().
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace orbfe {

struct UndistortParams {
  double fx, fy, cx, cy, ifx, ify;
  double k[8];
  int iters;
};

struct RectifyMapParams { double ir[9], fx, fy, u0, v0, k1, k2, p1, p2, k3, k4, k5, k6; int w, h; };

// frame f of nFrames at src + f * sFrame / dst + f * dFrame; strides in bytes
void launch_cvt_gray(hipStream_t s, const uint8_t* src, int w, int h, int sstride, size_t sFrame, int channels, int rgbOrder,
                     uint8_t* dst, int dstride, size_t dFrame, int nFrames);
void launch_distinctive(hipStream_t s, const uint8_t* desc, const int32_t* offsets, int nPoints, int32_t* best);
// the float maps (mstride floats per row) -> the rectifier's [h][pitch] arrays
void launch_remap_convert(hipStream_t s, const float* mx, const float* my, int mstride, int w, int h, int pitch, uint32_t* xy,
                          uint16_t* phase);
void launch_remap(hipStream_t s, const uint32_t* xy, const uint16_t* phase, int pitch, int w, int h, int nFrames,
                  const uint8_t* src, int sw, int sh, int sstride, size_t sFrame, uint8_t* dst, int dstride, size_t dFrame);
void launch_init_rectify_map(hipStream_t s, const RectifyMapParams& p, float* mapX, float* mapY);
void launch_undistort_points(hipStream_t s, const UndistortParams& p, const float* xy, int n, float* out);
void launch_undistort_keypoints(hipStream_t s, const UndistortParams& p, const float* kp, const int32_t* nKp, int capacity,
                                int nFrames, float* out);
void launch_stereo_from_rgbd(hipStream_t s, const float* kx, const float* ky, const float* kux, int n, const float* depthImg,
                             int stride, float mbf, float* uRight, float* depth);

}  // namespace orbfe
