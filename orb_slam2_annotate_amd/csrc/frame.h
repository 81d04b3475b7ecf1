// frame.h -- the resident Frame / KeyFrame handle (include/orbfe.h: orbfe_frame) as the searches read it, and how a call
// orders itself behind a frame's build.  The builds, orbfe_frame_set_featvec and the release are frames.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdint>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"

// ---------------------------------------------------------------------------------------------
// Device-resident Frame / KeyFrame operands (round 3).  The live system matches one key frame against 10-20
// neighbours (LocalMapping::CreateNewMapPoints / SearchInNeighbors, src/LocalMapping.cc:256-315, 517-573) and one
// frame against several candidates (Tracking::Relocalization, src/Tracking.cc:1478-1498): with host-pointer operands
// every call uploaded both frames' descriptors again.  orbfe_frame_upload moves what a frame contributes to ANY search
// -- keypoint arrays, descriptors, the 64 x 48 grid (built once), the FeatureVector's index list -- to the device once;
// the handle is immutable afterwards, so any thread may use it concurrently.
// ---------------------------------------------------------------------------------------------
struct orbfe_frame {
  int device = 0, n = 0;
  std::vector<float> hx, hy, hangle, hur;   // host copies: the claim loops and chi-square gates read them
  std::vector<int32_t> hoct;
  std::vector<uint8_t> hstereo;             // mvuRight[i] >= 0
  std::vector<uint32_t> nodeIds;            // FeatureVector (host side of the merge-walk)
  std::vector<int32_t> offsets;
  std::vector<uint32_t> hindices;
  orbfe_featvec fv = {};
  bool haveFv = false;
  orbfe::Slab slab;                         // one device allocation (from the slab pool)
  hipEvent_t ready = nullptr;               // recorded behind the upload + grid build; consumers on other streams wait for it
  mutable std::atomic<bool> settled{false}; // a consumer has synchronised behind `ready`: no further waits needed
  float *dx = nullptr, *dy = nullptr, *dangle = nullptr, *dur = nullptr;
  int32_t* doct = nullptr;
  uint8_t *ddesc = nullptr, *dstereo = nullptr;
  uint32_t *dkey = nullptr, *dindices = nullptr;
  int32_t* dcell = nullptr;
  std::vector<uint8_t> hdesc;               // (the host-pointer fallbacks of a view need it)
  orbfe_frame_view view = {};               // canonical view: host copies + resident = this
};

namespace orbfe {
inline const orbfe_frame_view* canon(const orbfe_frame_view* f) { return (f && f->resident) ? &f->resident->view : f; }

// a well-formed FeatureVector over n features: ascending node ids, ascending offsets from 0, indices below n
bool featvec_ok(const orbfe_featvec* f, int n);

// A search that reads a resident frame on ITS stream: ordered behind the frame's upload + grid build (which ran on the
// uploading thread's stream) by the frame's event -- the upload itself does not wait for the device.  Once any consumer
// has synchronised behind the event the frame is settled and nothing waits any more.
hipError_t frame_use(Arena* ar, const orbfe_frame* f);
void frames_settle();  // call after the stream of the call has been synchronised
// an entry point that returns early (a HIP error between frame_use and its synchronisation) must not leave frames on the
// list: they could be released before this thread's next call settles -- and writes to -- them
struct UnsettledScope {
  UnsettledScope();
  ~UnsettledScope();
};
}  // namespace orbfe
