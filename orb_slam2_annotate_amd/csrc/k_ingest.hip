// k_ingest.hip -- the per-pixel / per-map-point loops right next to the hot path (SURVEY.md 8(f)
// ranks 3-4): colour -> gray conversion in front of the extractor (Tracking::GrabImage*,
// src/Tracking.cc:176-262) and MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333).
// The kernels and their launchers (ingest_kernels.h); the entry points are ingest.hip.
#include <hip/hip_runtime.h>

#include "ingest_kernels.h"

using namespace orbfe;

namespace {

// cv::cvtColor(CV_RGB2GRAY etc.), 8U fixed point: (R*4899 + G*9617 + B*1868 + 2^13) >> 14.
// 4 output pixels per thread, one 32-bit store; 12 or 16 source bytes read as bytes (any stride).
__global__ __launch_bounds__(256) void k_cvt_gray(const uint8_t* __restrict__ src, int w, int h, int sstride,
                                                  size_t sFrame, int channels, int rgbOrder,
                                                  uint8_t* __restrict__ dst, int dstride, size_t dFrame) {
  const int x0 = (blockIdx.x * 256 + threadIdx.x) * 4, y = blockIdx.y, f = blockIdx.z;
  if (x0 >= w) return;
  const uint8_t* s = src + (size_t)f * sFrame + (size_t)y * sstride + (size_t)x0 * channels;
  uint8_t* d = dst + (size_t)f * dFrame + (size_t)y * dstride + x0;
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    if (x0 + k < w) {
      const uint8_t* p = s + k * channels;
      const int r = rgbOrder ? p[0] : p[2], g = p[1], b = rgbOrder ? p[2] : p[0];
      packed |= (uint32_t)((r * 4899 + g * 9617 + b * 1868 + (1 << 13)) >> 14) << (8 * k);
    }
  }
  if (x0 + 3 < w && ((reinterpret_cast<uintptr_t>(d) & 3) == 0)) {
    *reinterpret_cast<uint32_t*>(d) = packed;
  } else {
    for (int k = 0; k < 4 && x0 + k < w; k++) d[k] = (uint8_t)(packed >> (8 * k));
  }
}

// One workgroup per map point: n x n Hamming distances, per row the (size_t)(0.5*(n-1))-th order
// statistic via a 257-bin histogram, then the first row with the least median.
__global__ __launch_bounds__(256) void k_distinctive(const uint8_t* __restrict__ desc, const int32_t* __restrict__ offsets,
                                                     int32_t* __restrict__ best) {
  __shared__ int hist[4][257];
  __shared__ unsigned bestKey;  // median << 16 | row  (first minimum = smallest key)
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, m = blockIdx.x;
  const int b = offsets[m], n = offsets[m + 1] - b;
  if (tid == 0) bestKey = 0xffffffffu;
  __syncthreads();
  if (n <= 0) { if (tid == 0) best[m] = -1; return; }
  const int k = (int)(0.5 * (n - 1));
  for (int i = wave; i < n; i += 4) {  // one wave per row
    for (int t = lane; t < 257; t += 64) hist[wave][t] = 0;
    __builtin_amdgcn_wave_barrier();
    const uint4* pi = reinterpret_cast<const uint4*>(desc + (size_t)(b + i) * 32);
    const uint4 a0 = pi[0], a1 = pi[1];
    for (int j = lane; j < n; j += 64) {
      const uint4* pj = reinterpret_cast<const uint4*>(desc + (size_t)(b + j) * 32);
      const uint4 c0 = pj[0], c1 = pj[1];
      const int d = __popc(a0.x ^ c0.x) + __popc(a0.y ^ c0.y) + __popc(a0.z ^ c0.z) + __popc(a0.w ^ c0.w) +
                    __popc(a1.x ^ c1.x) + __popc(a1.y ^ c1.y) + __popc(a1.z ^ c1.z) + __popc(a1.w ^ c1.w);
      atomicAdd(&hist[wave][d], 1);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
      int acc = 0, med = 0;
      for (int t = 0; t < 257; t++) { acc += hist[wave][t]; if (acc > k) { med = t; break; } }
      atomicMin(&bestKey, ((unsigned)med << 16) | (unsigned)i);
    }
    __builtin_amdgcn_wave_barrier();
  }
  __syncthreads();
  if (tid == 0) best[m] = (int32_t)(bestKey & 0xffffu);
}


// ---------------------------------------------------------------------------------------------
// cv::remap(src, dst, M1 CV_32F, M2 CV_32F, INTER_LINEAR) -- the EuRoC stereo rectification in
// front of the extractor (Examples/Stereo/stereo_euroc.cc:97-98 builds the maps once, :136-137
// applies them to every frame).  The float maps are converted once, at create time, to what
// cv::remap converts them to for every tile of every frame: integer source coordinate saturated
// to int16 (packed sx | sy << 16) and a 10-bit sub-pixel phase (fy*32 + fx); the per-frame kernel
// then moves 6 map bytes + 1 source byte + 1 output byte per pixel.
// ---------------------------------------------------------------------------------------------

__device__ __forceinline__ int cvround_sse(float v) {  // cvtss2si: out of range / NaN -> INT_MIN
  if (!(v >= -2147483648.0f && v < 2147483648.0f)) return (int)0x80000000;
  return __float2int_rn(v);
}
__device__ __forceinline__ int sat_short(int v) { return v < -32768 ? -32768 : v > 32767 ? 32767 : v; }

__global__ __launch_bounds__(256) void k_remap_convert(const float* __restrict__ mx, const float* __restrict__ my,
                                                       int mstride, int w, int h, int pitch,
                                                       uint32_t* __restrict__ xy, uint16_t* __restrict__ phase) {
  const int x = blockIdx.x * 256 + threadIdx.x, y = blockIdx.y;
  if (x >= pitch) return;
  uint32_t c = 0x80008000u;  // padding columns: (-32768, -32768) -> border
  uint16_t p = 0;
  if (x < w) {
    const int isx = cvround_sse(mx[(size_t)y * mstride + x] * 32.0f), isy = cvround_sse(my[(size_t)y * mstride + x] * 32.0f);
    c = ((uint32_t)sat_short(isx >> 5) & 0xffffu) | ((uint32_t)sat_short(isy >> 5) << 16);
    p = (uint16_t)((isy & 31) * 32 + (isx & 31));
  }
  xy[(size_t)y * pitch + x] = c;
  phase[(size_t)y * pitch + x] = p;
}

// 4 output pixels per thread (one dword store); block = 64 x 4 threads = 256 x 4 pixels.  Blocks of
// one tile over all frames are adjacent in the grid, so the map tile is fetched from HBM once.
__global__ __launch_bounds__(256) void k_remap(const uint32_t* __restrict__ xy, const uint16_t* __restrict__ phase,
                                               int pitch, int w, int h, int tilesX, int nFrames,
                                               const uint8_t* __restrict__ src, int sw, int sh, int sstride,
                                               size_t sFrame, uint8_t* __restrict__ dst, int dstride, size_t dFrame) {
  const int f = blockIdx.x % nFrames, tile = blockIdx.x / nFrames;
  const int x0 = ((tile % tilesX) * 64 + (threadIdx.x & 63)) * 4, y = (tile / tilesX) * 4 + (threadIdx.x >> 6);
  if (x0 >= w || y >= h) return;
  const uint4 c4 = *reinterpret_cast<const uint4*>(xy + (size_t)y * pitch + x0);
  const uint2 p4 = *reinterpret_cast<const uint2*>(phase + (size_t)y * pitch + x0);
  const uint32_t cs[4] = {c4.x, c4.y, c4.z, c4.w};
  const uint32_t ps[4] = {p4.x & 0xffffu, p4.x >> 16, p4.y & 0xffffu, p4.y >> 16};
  const uint8_t* S0 = src + (size_t)f * sFrame;
  const unsigned width1 = (unsigned)(sw - 1 > 0 ? sw - 1 : 0), height1 = (unsigned)(sh - 1 > 0 ? sh - 1 : 0);
  uint32_t packed = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int sx = (int)(int16_t)(cs[k] & 0xffffu), sy = (int)(int16_t)(cs[k] >> 16);
    const int fx = (int)(ps[k] & 31u), fy = (int)(ps[k] >> 5);
    int v0 = 0, v1 = 0, v2 = 0, v3 = 0;
    if ((unsigned)sx < width1 && (unsigned)sy < height1) {
      const uint8_t* S = S0 + (size_t)sy * sstride + sx;
      v0 = S[0]; v1 = S[1]; v2 = S[sstride]; v3 = S[sstride + 1];
    } else if (!(sx >= sw || sx + 1 < 0 || sy >= sh || sy + 1 < 0)) {
      const bool x0in = sx >= 0 && sx < sw, x1in = sx + 1 >= 0 && sx + 1 < sw;
      const bool y0in = sy >= 0 && sy < sh, y1in = sy + 1 >= 0 && sy + 1 < sh;
      if (x0in && y0in) v0 = S0[(size_t)sy * sstride + sx];
      if (x1in && y0in) v1 = S0[(size_t)sy * sstride + sx + 1];
      if (x0in && y1in) v2 = S0[(size_t)(sy + 1) * sstride + sx];
      if (x1in && y1in) v3 = S0[(size_t)(sy + 1) * sstride + sx + 1];
    }
    // sum of v*w with w = (32-fy)(32-fx)*32 ...; (32 t + 2^14) >> 15 == (t + 512) >> 10
    const int t = (v0 * (32 - fx) + v1 * fx) * (32 - fy) + (v2 * (32 - fx) + v3 * fx) * fy;
    packed |= (uint32_t)((t + 512) >> 10) << (8 * k);
  }
  uint8_t* d = dst + (size_t)f * dFrame + (size_t)y * dstride + x0;
  if (x0 + 3 < w && ((reinterpret_cast<uintptr_t>(d) & 3) == 0)) {
    *reinterpret_cast<uint32_t*>(d) = packed;
  } else {
    for (int k = 0; k < 4 && x0 + k < w; k++) d[k] = (uint8_t)(packed >> (8 * k));
  }
}


// ---------------------------------------------------------------------------------------------
// Frame::UndistortKeyPoints / ComputeImageBounds (cv::undistortPoints with P = K,
// src/Frame.cc:443-510) and Frame::ComputeStereoFromRGBD (src/Frame.cc:689-713): the per-keypoint
// loops between the extractor and the matchers.  Double precision, no FMA contraction (the
// library is built with -ffp-contract=off), IEEE division: bit-identical to the host arithmetic.
// ---------------------------------------------------------------------------------------------

__device__ __forceinline__ void undistort_one(const UndistortParams& p, float xin, float yin, float* xo, float* yo) {
  double x = (double)xin, y = (double)yin, x0, y0;
  x0 = x = (x - p.cx) * p.ifx;
  y0 = y = (y - p.cy) * p.ify;
  for (int j = 0; j < p.iters; j++) {
    const double r2 = x * x + y * y;
    const double icdist =
        (1 + ((p.k[7] * r2 + p.k[6]) * r2 + p.k[5]) * r2) / (1 + ((p.k[4] * r2 + p.k[1]) * r2 + p.k[0]) * r2);
    const double deltaX = 2 * p.k[2] * x * y + p.k[3] * (r2 + 2 * x * x);
    const double deltaY = p.k[2] * (r2 + 2 * y * y) + 2 * p.k[3] * x * y;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  const double xx = p.fx * x + 0.0 * y + p.cx;  // RR = P * I = K
  const double yy = 0.0 * x + p.fy * y + p.cy;
  const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
  *xo = (float)(xx * ww);
  *yo = (float)(yy * ww);
}

__global__ __launch_bounds__(256) void k_undistort_points(UndistortParams p, const float* __restrict__ xy, int n,
                                                          float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  undistort_one(p, xy[2 * i], xy[2 * i + 1], &out[2 * i], &out[2 * i + 1]);
}

// mvKeysUn for a device-resident extractor batch: 28-byte records copied, pt replaced
__global__ __launch_bounds__(256) void k_undistort_keypoints(UndistortParams p, const float* __restrict__ kp,
                                                             const int32_t* __restrict__ nKp, int capacity,
                                                             float* __restrict__ out) {
  const int f = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nKp[f] || i >= capacity) return;
  const float* s = kp + ((size_t)f * capacity + i) * 7;
  float* d = out + ((size_t)f * capacity + i) * 7;
  float x, y;
  undistort_one(p, s[0], s[1], &x, &y);
  d[0] = x; d[1] = y;
#pragma unroll
  for (int k = 2; k < 7; k++) d[k] = s[k];
}

__global__ __launch_bounds__(256) void k_stereo_from_rgbd(const float* __restrict__ kx, const float* __restrict__ ky,
                                                          const float* __restrict__ kux, int n,
                                                          const float* __restrict__ depthImg, int stride, float mbf,
                                                          float* __restrict__ uRight, float* __restrict__ depth) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float d = depthImg[(size_t)(int)ky[i] * stride + (int)kx[i]];
  float ur = -1.0f, dd = -1.0f;
  if (d > 0) { dd = d; ur = kux[i] - mbf / d; }
  uRight[i] = ur;
  depth[i] = dd;
}

// cv::initUndistortRectifyMap(K, D, R, P[:3,:3], size, CV_32F, M1, M2) as Examples/Stereo/stereo_euroc.cc:97-98 calls it,
// once at start-up: the two float maps orbfe_rectifier_create takes.  One THREAD per map row -- the reference walks a row
// with running sums (_x += ir[0], ...), so a row is a sequential chain in double precision; rows are independent.  No FMA
// contraction (the build's -ffp-contract=off), IEEE division.
__global__ __launch_bounds__(64) void k_init_rectify_map(const RectifyMapParams p, float* __restrict__ mapX, float* __restrict__ mapY) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= p.h) return;
  double _x = __dadd_rn(__dmul_rn((double)i, p.ir[1]), p.ir[2]), _y = __dadd_rn(__dmul_rn((double)i, p.ir[4]), p.ir[5]),
         _w = __dadd_rn(__dmul_rn((double)i, p.ir[7]), p.ir[8]);
  float* mx = mapX + (size_t)i * p.w;
  float* my = mapY + (size_t)i * p.w;
  for (int j = 0; j < p.w; j++) {
    const double ww = __ddiv_rn(1.0, _w), x = __dmul_rn(_x, ww), y = __dmul_rn(_y, ww);
    const double x2 = __dmul_rn(x, x), y2 = __dmul_rn(y, y);
    const double r2 = __dadd_rn(x2, y2), _2xy = __dmul_rn(__dmul_rn(2.0, x), y);
    const double num = __dadd_rn(1.0, __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(p.k3, r2), p.k2), r2), p.k1), r2));
    const double den = __dadd_rn(1.0, __dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(p.k6, r2), p.k5), r2), p.k4), r2));
    const double kr = __ddiv_rn(num, den);
    const double xd = __dadd_rn(__dadd_rn(__dmul_rn(x, kr), __dmul_rn(p.p1, _2xy)), __dmul_rn(p.p2, __dadd_rn(r2, __dmul_rn(2.0, x2))));
    const double yd = __dadd_rn(__dadd_rn(__dmul_rn(y, kr), __dmul_rn(p.p1, __dadd_rn(r2, __dmul_rn(2.0, y2)))), __dmul_rn(p.p2, _2xy));
    mx[j] = (float)__dadd_rn(__dmul_rn(p.fx, xd), p.u0);
    my[j] = (float)__dadd_rn(__dmul_rn(p.fy, yd), p.v0);
    _x = __dadd_rn(_x, p.ir[0]); _y = __dadd_rn(_y, p.ir[3]); _w = __dadd_rn(_w, p.ir[6]);
  }
}
}  // namespace

namespace orbfe {

void launch_cvt_gray(hipStream_t s, const uint8_t* src, int w, int h, int sstride, size_t sFrame, int channels, int rgbOrder,
                     uint8_t* dst, int dstride, size_t dFrame, int nFrames) {
  hipLaunchKernelGGL(k_cvt_gray, dim3((w + 1023) / 1024, h, nFrames), dim3(256), 0, s, src, w, h, sstride, sFrame, channels,
                     rgbOrder, dst, dstride, dFrame);
}

void launch_distinctive(hipStream_t s, const uint8_t* desc, const int32_t* offsets, int nPoints, int32_t* best) {
  hipLaunchKernelGGL(k_distinctive, dim3(nPoints), dim3(256), 0, s, desc, offsets, best);
}

void launch_remap_convert(hipStream_t s, const float* mx, const float* my, int mstride, int w, int h, int pitch, uint32_t* xy,
                          uint16_t* phase) {
  hipLaunchKernelGGL(k_remap_convert, dim3((pitch + 255) / 256, h), dim3(256), 0, s, mx, my, mstride, w, h, pitch, xy, phase);
}

void launch_remap(hipStream_t s, const uint32_t* xy, const uint16_t* phase, int pitch, int w, int h, int nFrames,
                  const uint8_t* src, int sw, int sh, int sstride, size_t sFrame, uint8_t* dst, int dstride, size_t dFrame) {
  const int tilesX = (w + 255) / 256, tilesY = (h + 3) / 4;
  hipLaunchKernelGGL(k_remap, dim3((unsigned)tilesX * tilesY * nFrames), dim3(256), 0, s, xy, phase, pitch, w, h, tilesX, nFrames,
                     src, sw, sh, sstride, sFrame, dst, dstride, dFrame);
}

void launch_init_rectify_map(hipStream_t s, const RectifyMapParams& p, float* mapX, float* mapY) {
  hipLaunchKernelGGL(k_init_rectify_map, dim3((p.h + 63) / 64), dim3(64), 0, s, p, mapX, mapY);
}

void launch_undistort_points(hipStream_t s, const UndistortParams& p, const float* xy, int n, float* out) {
  hipLaunchKernelGGL(k_undistort_points, dim3((n + 255) / 256), dim3(256), 0, s, p, xy, n, out);
}

void launch_undistort_keypoints(hipStream_t s, const UndistortParams& p, const float* kp, const int32_t* nKp, int capacity,
                                int nFrames, float* out) {
  hipLaunchKernelGGL(k_undistort_keypoints, dim3((capacity + 255) / 256, nFrames), dim3(256), 0, s, p, kp, nKp, capacity, out);
}

void launch_stereo_from_rgbd(hipStream_t s, const float* kx, const float* ky, const float* kux, int n, const float* depthImg,
                             int stride, float mbf, float* uRight, float* depth) {
  hipLaunchKernelGGL(k_stereo_from_rgbd, dim3((n + 255) / 256), dim3(256), 0, s, kx, ky, kux, n, depthImg, stride, mbf, uRight,
                     depth);
}

}  // namespace orbfe

