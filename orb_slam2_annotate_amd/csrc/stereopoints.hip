// stereopoints.hip -- host side of stereo and RGB-D map-point creation (include/orbfe.h: orbfe_stereo_points_select,
// orbfe_count_close_points, orbfe_create_stereo_points; kernel: k_stereopoints.hip; host arithmetic:
// stereopoints_host.h).  References: Tracking::StereoInitialization (src/Tracking.cc:563-578), Tracking::UpdateLastFrame
// (:899-949), Tracking::CreateNewKeyFrame (:1182-1234), Tracking::NeedNewKeyFrame (:1100-1114).
//
// The resident call takes the graph's serialisation (modes ALL and KEYFRAME), then the map-point table's, stages through
// the graph's arena -- in mode TEMPORAL, which names no graph, through the calling thread's -- and is complete on return.
// Every operand is checked before anything is enqueued.  The kernel writes the map-point table alone; what the new points
// mean to the graph (set_points, AddObservation, AddMapPoint) is applied to the graph's mirror afterwards, in creation
// order, by the mirror's own mutators, and reaches the device with the graph's next reading call like any other mutation.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "frame.h"
#include "host_internal.h"
#include "obsgraph_handle.h"
#include "obsgraph_host.h"
#include "stereopoints_host.h"
#include "stereopoints_kernels.h"

using namespace orbfe;

extern "C" int orbfe_stereo_points_select(int n, const float* x, const float* y, const int32_t* octave, const float* depth,
                                          const uint8_t* occupied, const uint8_t* stale, const orbfe_camera_pose* pose, float th_depth, int mode,
                                          const float* scale_factors, int n_levels, const float* centre, int capacity, int32_t* created_idx,
                                          float* pos, float* normal, float* min_dist, float* max_dist, uint8_t* cleared, int32_t* n_created,
                                          int32_t* n_walked) {
  bool over = false;
  if (const char* e = stereo_points_select(n, x, y, octave, depth, occupied, stale, pose, th_depth, mode, scale_factors, n_levels, centre, capacity,
                                           created_idx, pos, normal, min_dist, max_dist, cleared, n_created, n_walked, &over))
    return fail(over ? ORBFE_ERR_CAPACITY : ORBFE_ERR_INVALID, std::string("stereo_points_select: ") + e);
  return ORBFE_OK;
}

extern "C" int orbfe_count_close_points(int n, const float* depth, const uint8_t* has_point, const uint8_t* outlier, float th_depth,
                                        int32_t* n_tracked_close, int32_t* n_non_tracked_close) {
  if (const char* e = count_close_points(n, depth, has_point, outlier, th_depth, n_tracked_close, n_non_tracked_close))
    return fail(ORBFE_ERR_INVALID, std::string("count_close_points: ") + e);
  return ORBFE_OK;
}

extern "C" int orbfe_create_stereo_points(orbfe_mappoints* mp, orbfe_obsgraph* g, const orbfe_frame* F, int kf_slot,
                                          const orbfe_camera_pose* pose, int n, const float* depth, const uint8_t* occupied,
                                          const uint8_t* stale, float th_depth, int mode, const float* scale_factors, int n_levels,
                                          const int32_t* new_slot, int capacity, int32_t* created_idx, int32_t* created_slot, uint8_t* cleared,
                                          int32_t* n_created, int32_t* n_walked) {
  const std::string fn = "create_stereo_points: ";
  auto invalid = [&](const char* what) { return fail(ORBFE_ERR_INVALID, fn + what); };
  if (!mp || !F || !n_created || !n_walked) return invalid("NULL argument");
  if (n != F->n) return invalid("n is not the resident frame's keypoint count");
  if (capacity < 0) return invalid("negative capacity");
  if (const char* e = sp_check_operands(n, F->hoct.data(), depth, occupied, stale, pose, mode, scale_factors, n_levels)) return invalid(e);
  const bool temporal = mode == ORBFE_STEREO_TEMPORAL;
  if (!temporal && !g) return invalid("modes ALL and KEYFRAME need the observation graph");
  if (temporal) g = nullptr;  // the temporal points are no map points: the graph never hears of them
  if (capacity > 0 && (!new_slot || !created_idx || !created_slot)) return invalid("NULL slot or output list");
  if (n > 0 && !cleared) return invalid("NULL cleared");
  const int mpCap = orbfe_mappoints_capacity(mp), device = mappoints_device(mp);
  if (F->device != device) return invalid("the frame and the map-point table are on different devices");
  for (int j = 0; j < capacity; j++)
    if (new_slot[j] < 0 || new_slot[j] >= mpCap) return invalid("a new slot is outside [0, capacity of the table)");
  {  // (distinct slots: what ObsGraphMirror::check_new_points below takes for granted)
    std::vector<int32_t> sorted(new_slot, new_slot + capacity);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return invalid("a new slot is named twice");
  }
  std::unique_lock<std::mutex> lk;
  if (g) {
    lk = std::unique_lock<std::mutex>(g->m);
    const ObsGraphMirror& h = g->h;
    if (g->device != device) return invalid("the graph and the map-point table are on different devices");
    // what the mirror's mutators could refuse after the kernel has written the table: asked of the mirror itself, now
    if (const char* e = h.check_new_points(capacity, new_slot, kf_slot, n)) return invalid(e);
  }
  *n_created = *n_walked = 0;
  for (int i = 0; i < n; i++) cleared[i] = 0;
  int m = 0;
  for (int i = 0; i < n; i++) m += sp_candidate(sp_bits(depth[i])) ? 1 : 0;
  if (m == 0) return ORBFE_OK;

  MapPointsLock lock(mp);  // the table's own calls have completed and stay out for the scope
  if (lock.rc) return lock.rc;
  const size_t nK = (size_t)n, nSlots = (size_t)std::min(capacity, n), L = (size_t)n_levels;
  StereoPointsArgs a;
  a.n = n; a.mode = mode; a.nLevels = n_levels; a.capacity = capacity;
  a.sortN = 64;
  while (a.sortN < m) a.sortN <<= 1;
  a.thDepth = th_depth; a.invfx = 1.0f / pose->fx; a.invfy = 1.0f / pose->fy;  // Frame::invfx, invfy
  a.pose = *pose;
  const float* C = temporal ? pose->Ow : g->h.kfs[(size_t)kf_slot].ow;
  a.centre[0] = C[0]; a.centre[1] = C[1]; a.centre[2] = C[2];
  a.flags = temporal ? 0 : ORBFE_MP_OBSERVED;
  a.x = F->dx; a.y = F->dy; a.octave = F->doct; a.desc = F->ddesc;
  float *dDepth, *dScale;
  uint8_t *dOcc = nullptr, *dStale = nullptr;
  int32_t* dSlot;
  auto stage = [&](Arena* s) -> hipError_t {
    TRY(up(s, &dDepth, depth, nK));
    if (occupied && mode != ORBFE_STEREO_ALL) TRY(up(s, &dOcc, occupied, nK));
    if (stale && mode == ORBFE_STEREO_KEYFRAME) TRY(up(s, &dStale, stale, nK));
    TRY(up(s, &dSlot, new_slot, nSlots));
    TRY(up(s, &dScale, scale_factors, L));
    open_span(s);  // what comes back, in one copy
    a.header = carve<int32_t>(s, 2);
    a.createdIdx = carve<int32_t>(s, nSlots ? nSlots : 1);
    a.cleared = carve<uint8_t>(s, nK);
    return close_span(s);
  };
  Arena* ar;
  if (g) {
    ar = &g->arena;
    HIPCHK(arena_stage(ar, device, stage));
  } else {
    HIPCHK(arena_stage(device, &ar, stage));
  }
  a.depth = dDepth; a.occupied = dOcc; a.stale = dStale; a.newSlot = dSlot; a.scale = dScale;
  UnsettledScope unsettled;
  HIPCHK(frame_use(ar, F));
  HIPCHK(flush(ar));
  launch_stereo_points(ar->stream, *lock.table, a);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  frames_settle();
  const int32_t* header = mirror_of(ar, a.header);
  const int created = header[0], walked = header[1];
  if (created < 0 || walked < created || walked > m) return fail(ORBFE_ERR_HIP, fn + "the device returned an impossible count");
  *n_created = created;
  *n_walked = walked;
  if (created > capacity) return fail(ORBFE_ERR_CAPACITY, fn + "more points are created than `capacity` (see *n_created); nothing was changed");
  const size_t cnt = (size_t)created;
  std::memcpy(created_idx, mirror_of(ar, a.createdIdx), cnt * 4);
  std::memcpy(created_slot, new_slot, cnt * 4);
  std::memcpy(cleared, mirror_of(ar, a.cleared), nK);
  if (!g || cnt == 0) return ORBFE_OK;
  // the map bookkeeping of :1216-1221 on the graph's mirror, in creation order
  ObsGraphMirror& h = g->h;
  std::vector<uint8_t> zero(cnt, 0), oct(cnt), stereo(cnt);
  std::vector<int32_t> kf(cnt, kf_slot);
  std::vector<uint16_t> idx(cnt);
  for (size_t j = 0; j < cnt; j++) {
    const int i = created_idx[j];
    if (i < 0 || i >= n) return fail(ORBFE_ERR_HIP, fn + "the device returned an impossible index");
    idx[j] = (uint16_t)i;
    oct[j] = (uint8_t)F->hoct[(size_t)i];
    stereo[j] = F->hstereo.empty() ? 0 : F->hstereo[(size_t)i];  // the frame's own mvuRight >= 0
  }
  bool full = false;
  const char* e = h.set_points(created, new_slot, zero.data(), kf.data());                                  // MapPoint(x3D, pKF, mpMap)
  if (!e) e = h.add_observations(created, new_slot, kf.data(), idx.data(), oct.data(), stereo.data(), &full);  // AddObservation(pKF, i)
  if (!e && h.kfRowWidth) e = h.assign_keyframe_points(created, kf.data(), idx.data(), new_slot);            // pKF->AddMapPoint(pNewMP, i)
  // check_new_points() accepted them before the launch: a refusal here means the two lists have parted
  if (e || full) return fail(ORBFE_ERR_HIP, fn + "the graph's mirror refused points its own check accepted: " + (e ? e : "a row is full"));
  return ORBFE_OK;
}
