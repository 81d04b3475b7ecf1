// obsgraph_handle.h -- struct orbfe_obsgraph and what its host files share (obsgraph.hip: the observation rows;
// kfpoints.hip: the key-frame rows; obsdesc.hip: the key frames' descriptors; loopcorrect.hip: the loop correction).
// Everything here is called with the handle locked.  The handle owns an arena (arena.h): its calls stage through
// arena_stage(&g->arena, g->device, stage) and run on g->arena.stream, whichever thread makes them.
#pragma once
#include <hip/hip_runtime.h>

#include <mutex>
#include <string>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "obsgraph_host.h"
#include "obsgraph_kernels.h"

struct orbfe_obsgraph {
  int device = 0;
  std::mutex m;  // a handle serialises its own calls
  orbfe::ObsGraphMirror h;
  orbfe::Slab table;  // empty until the first call that needs the device
  orbfe::ObsGraphDevice d{};
  // KeyFrame::mvpMapPoints: a slab of its own, empty until the first device call after enable_keyframe_points
  orbfe::Slab kfTable;
  orbfe::KfPointsDevice kd{};
  // KeyFrame::mDescriptors: a slab of its own, empty until the first set_keyframe_descriptors*; no host copy of the bytes
  orbfe::Slab descTable;
  orbfe::KfDescDevice dd{};
  // kf slot -> place in the list of a loop-correction call (loopcorrect.hip): kf_capacity int32, -1 everywhere between
  // calls; empty until the first such call
  orbfe::DevBuf<int32_t> kfRank;
  // the handle's stream (made by the first call that touches the device), workspace and pinned mirror
  orbfe::Arena arena;
};

namespace orbfe {

constexpr size_t kObsFlushChunkBytes = (size_t)8 << 20;

// what every call that reads the table on the device starts with: device, stream, the slab, the marked rows written
int obs_ready(orbfe_obsgraph* g);
int obs_invalid(const char* fn, const char* what);
// kfpoints.hip: obs_ready, then the key-frame rows' own slab and their marked rows (the rows enabled)
int obs_kf_ready(orbfe_obsgraph* g);

}  // namespace orbfe
