// stereopoints_kernels.h -- launch interface of k_stereopoints.hip (host side: stereopoints.hip).
#pragma once
#include <hip/hip_runtime.h>

#include "match_kernels.h"

namespace orbfe {

// the two LDS sizes of k_stereo_points: the candidates' 64-bit keys are sorted in one workgroup's LDS, 16 KiB of keys for
// up to 2048 candidates, 128 KiB -- of the CU's 160 KiB -- for up to 16384
constexpr int kSpSmallKeys = 2048, kSpMaxKeys = 16384, kSpThreads = 1024;

// One orbfe_create_stereo_points call.  x / y / octave / desc: the resident frame's arrays (n keypoints); depth [n];
// occupied / stale [n] or NULL (none set); newSlot [min(capacity, n)]; scale [nLevels].  sortN: a power of two, at least 64
// and at least the number of candidates (depth > 0), at most kSpMaxKeys.  header [2]: created, walked; createdIdx
// [min(capacity, n)] and the table rows are written only when created <= capacity; cleared [n].
struct StereoPointsArgs {
  int n, mode, nLevels, capacity, sortN;
  float thDepth, invfx, invfy;
  orbfe_camera_pose pose;
  float centre[3];
  int flags;
  const float *x, *y;
  const int32_t* octave;
  const uint8_t* desc;
  const float* depth;
  const uint8_t *occupied, *stale;
  const int32_t* newSlot;
  const float* scale;
  int32_t *header, *createdIdx;
  uint8_t* cleared;
};
void launch_stereo_points(hipStream_t s, const MapPointsDevice& table, const StereoPointsArgs& a);

}  // namespace orbfe
