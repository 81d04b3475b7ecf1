// tripoints.hip -- host side of the triangulated map points of LocalMapping::CreateNewMapPoints (include/orbfe.h:
// orbfe_triangulated_points_select, orbfe_create_triangulated_points; kernels: k_tripoints.hip; host arithmetic:
// tripoints_host.h; argument checks and the pair list: triangulate_host.h).  Reference: src/LocalMapping.cc:283-501.
//
// The resident call takes the graph's serialisation, then the map-point table's, stages through the graph's arena and is
// complete on return.  Every operand is checked before anything is enqueued.  The kernels write the map-point table alone;
// what the new points mean to the graph (the MapPoint constructor, AddObservation twice, AddMapPoint twice, :484-492) is
// applied to the graph's mirror afterwards, in creation order, by the mirror's own mutators, and reaches the device with
// the graph's next reading call like any other mutation.
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
#include "tripoints_host.h"
#include "tripoints_kernels.h"

using namespace orbfe;

static_assert(kTpMaxNeighbours == kTriHostMaxNeighbours, "the per-neighbour counts of k_tri_points_place cover every neighbour");

extern "C" int orbfe_triangulated_points_select(int n1, int n_neighbours, const int32_t* match12, const uint8_t* status, const float* x3d,
                                                int64_t kf1_id, const int64_t* kf2_id, const float* centre1, const float* centre2,
                                                const int32_t* octave1, const float* scale_factors, int n_levels, int capacity,
                                                int32_t* created_k, int32_t* created_i1, int32_t* created_i2, float* pos, float* normal,
                                                float* min_dist, float* max_dist, uint8_t* desc_from, int32_t* n_created) {
  bool over = false;
  if (const char* e = triangulated_points_select(n1, n_neighbours, match12, status, x3d, kf1_id, kf2_id, centre1, centre2, octave1, scale_factors,
                                                 n_levels, capacity, created_k, created_i1, created_i2, pos, normal, min_dist, max_dist, desc_from,
                                                 n_created, &over))
    return fail(over ? ORBFE_ERR_CAPACITY : ORBFE_ERR_INVALID, std::string("triangulated_points_select: ") + e);
  return ORBFE_OK;
}

extern "C" int orbfe_create_triangulated_points(orbfe_mappoints* mp, orbfe_obsgraph* g, const orbfe_frame* kf1, int kf1_slot,
                                                const orbfe_keyframe_camera* cam1, int n_neighbours, const orbfe_frame* const* kf2,
                                                const int32_t* kf2_slot, const orbfe_keyframe_camera* cam2, const int32_t* match12,
                                                const float* scale_factors, const float* level_sigma2, int n_levels, float ratio_factor,
                                                const int32_t* new_slot, int capacity, int32_t* created_k, int32_t* created_i1,
                                                int32_t* created_i2, int32_t* created_slot, uint8_t* status,
                                                int32_t* n_created_per_neighbour, int32_t* n_created) {
  const std::string fn = "create_triangulated_points: ";
  auto invalid = [&](const char* what) { return fail(ORBFE_ERR_INVALID, fn + what); };
  const int K = n_neighbours;
  if (!mp || !g || !kf1 || !n_created) return invalid("NULL argument");
  if (K < 0 || K > kTriHostMaxNeighbours) return invalid("n_neighbours outside [0, 64]");
  if (K > 0 && (!kf2 || !kf2_slot || !n_created_per_neighbour)) return invalid("NULL array");
  if (capacity < 0) return invalid("negative capacity");
  if (capacity > 0 && (!new_slot || !created_k || !created_i1 || !created_i2 || !created_slot)) return invalid("NULL slot or output list");
  std::vector<const orbfe_frame_view*> h2((size_t)K);
  for (int k = 0; k < K; k++) {
    if (!kf2[k]) return invalid("NULL neighbour");
    h2[(size_t)k] = &kf2[k]->view;
  }
  const orbfe_frame_view* h1 = &kf1->view;
  if (const char* e = triangulate_check_inputs(h1, cam1, K, h2.data(), cam2, match12, scale_factors, level_sigma2, n_levels)) return invalid(e);
  const int n1 = kf1->n;
  {
    std::vector<uint8_t> seen;
    for (int k = 0; k < K; k++)
      if (tp_i2_twice(n1, match12 + (size_t)k * n1, kf2[k]->n, &seen)) return invalid("a keypoint of a neighbour is matched twice");
  }
  const int mpCap = orbfe_mappoints_capacity(mp), device = mappoints_device(mp);
  if (kf1->device != device) return invalid("key frame 1 and the map-point table are on different devices");
  for (int k = 0; k < K; k++)
    if (kf2[k]->device != device) return invalid("a neighbour and the map-point table are on different devices");
  for (int j = 0; j < capacity; j++)
    if (new_slot[j] < 0 || new_slot[j] >= mpCap) return invalid("a new slot is outside [0, capacity of the table)");
  {  // (distinct slots: what ObsGraphMirror::check_new_pair_points below takes for granted)
    std::vector<int32_t> sorted(new_slot, new_slot + capacity);
    std::sort(sorted.begin(), sorted.end());
    if (std::adjacent_find(sorted.begin(), sorted.end()) != sorted.end()) return invalid("a new slot is named twice");
  }
  std::vector<int32_t> kfSlots((size_t)K + 1), kfN((size_t)K + 1);
  kfSlots[0] = kf1_slot; kfN[0] = n1;
  for (int k = 0; k < K; k++) { kfSlots[1 + (size_t)k] = kf2_slot[k]; kfN[1 + (size_t)k] = kf2[k]->n; }
  std::unique_lock<std::mutex> lk(g->m);
  ObsGraphMirror& h = g->h;
  if (g->device != device) return invalid("the graph and the map-point table are on different devices");
  // what the mirror's mutators could refuse after the kernels have written the table: asked of the mirror itself, now
  if (const char* e = h.check_new_pair_points(capacity, new_slot, K + 1, kfSlots.data(), kfN.data())) return invalid(e);

  *n_created = 0;
  for (int k = 0; k < K; k++) n_created_per_neighbour[k] = 0;
  if (status && K > 0 && n1 > 0) std::memset(status, 0, (size_t)K * (size_t)n1);
  std::vector<TriangulatePair> pairs;
  triangulate_pairs(h1, cam1, K, h2.data(), cam2, match12, &pairs);
  if (pairs.empty()) return ORBFE_OK;

  MapPointsLock lock(mp);  // the table's own calls have completed and stay out for the scope
  if (lock.rc) return lock.rc;
  const size_t nPairs = pairs.size(), nSlots = std::min((size_t)capacity, nPairs);
  std::vector<TriCamera> cams((size_t)K + 1);
  cams[0] = tri_camera(cam1);
  for (int k = 0; k < K; k++) cams[1 + (size_t)k] = tri_camera(cam2 + k);
  std::vector<TriangulateFrame> frames((size_t)K + 1);
  std::vector<TriPointsKeyFrame> kfs((size_t)K + 1);
  const int64_t id1 = h.kfs[(size_t)kf1_slot].id;
  for (size_t j = 0; j <= (size_t)K; j++) {
    const orbfe_frame* F = j ? kf2[j - 1] : kf1;
    const ObsKeyFrame& mk = h.kfs[(size_t)kfSlots[j]];  // the mirror is the truth for centre and mnId
    frames[j].x = F->dx; frames[j].y = F->dy; frames[j].octave = F->doct; frames[j].ur = F->view.u_right ? F->dur : nullptr;
    kfs[j].desc = F->ddesc;
    kfs[j].ow[0] = mk.ow[0]; kfs[j].ow[1] = mk.ow[1]; kfs[j].ow[2] = mk.ow[2];
    kfs[j].first = j && mk.id < id1 ? 1 : 0;
  }
  TriPointsArgs a = {};
  a.tri.nPairs = (int)nPairs; a.tri.n1 = n1; a.tri.ratioFactor = ratio_factor;
  a.nLevels = n_levels; a.capacity = capacity; a.flags = ORBFE_MP_OBSERVED;
  a.octave1 = kf1->doct;
  auto stage = [&](Arena* s) -> hipError_t {
    TriangulatePair* dPairs;
    TriCamera* dCams;
    TriangulateFrame* dFrames;
    TriPointsKeyFrame* dKfs;
    float *dSf, *dSg;
    int32_t* dSlot;
    TRY(up(s, &dPairs, pairs.data(), nPairs));
    TRY(up(s, &dCams, cams.data(), cams.size()));
    TRY(up(s, &dFrames, frames.data(), frames.size()));
    TRY(up(s, &dKfs, kfs.data(), kfs.size()));
    TRY(up(s, &dSf, scale_factors, (size_t)n_levels));
    TRY(up(s, &dSg, level_sigma2, (size_t)n_levels));
    TRY(up(s, &dSlot, new_slot, nSlots));
    TRY(up_fill(s, &a.tri.winner, (size_t)n1, 0x7f));  // kTriangulateNoWinner
    a.pairPos = carve<float4>(s, nPairs);               // workspace: stays on the device
    open_span(s);                                       // what comes back, in one copy
    a.header = carve<int32_t>(s, 1 + kTpMaxNeighbours);
    a.createdK = carve<int32_t>(s, nSlots ? nSlots : 1);
    a.createdI1 = carve<int32_t>(s, nSlots ? nSlots : 1);
    a.createdI2 = carve<int32_t>(s, nSlots ? nSlots : 1);
    a.pairStatus = carve<uint8_t>(s, nPairs);
    TRY(close_span(s));
    a.tri.pairs = dPairs; a.tri.cams = dCams; a.tri.frames = dFrames; a.tri.scaleFactors = dSf; a.tri.levelSigma2 = dSg;
    a.kfs = dKfs; a.newSlot = dSlot;
    return hipSuccess;
  };
  Arena* ar = &g->arena;
  HIPCHK(arena_stage(ar, device, stage));
  UnsettledScope unsettled;
  HIPCHK(frame_use(ar, kf1));
  for (int k = 0; k < K; k++) HIPCHK(frame_use(ar, kf2[k]));
  HIPCHK(flush(ar));
  launch_tri_points(ar->stream, *lock.table, a);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  frames_settle();
  const int32_t* header = mirror_of(ar, a.header);
  const int created = header[0];
  if (created < 0 || (size_t)created > nPairs || created > n1) return fail(ORBFE_ERR_HIP, fn + "the device returned an impossible count");
  *n_created = created;
  for (int k = 0; k < K; k++) n_created_per_neighbour[k] = header[1 + k];
  if (status) {
    const uint8_t* ps = mirror_of(ar, a.pairStatus);
    for (size_t p = 0; p < nPairs; p++) status[(size_t)pairs[p].k * (size_t)n1 + (size_t)pairs[p].i1] = ps[p];
  }
  if (created > capacity) return fail(ORBFE_ERR_CAPACITY, fn + "more points are created than `capacity` (see *n_created); nothing was changed");
  const size_t cnt = (size_t)created;
  if (cnt == 0) return ORBFE_OK;
  std::memcpy(created_k, mirror_of(ar, a.createdK), cnt * 4);
  std::memcpy(created_i1, mirror_of(ar, a.createdI1), cnt * 4);
  std::memcpy(created_i2, mirror_of(ar, a.createdI2), cnt * 4);
  std::memcpy(created_slot, new_slot, cnt * 4);
  // the map bookkeeping of :484-492 on the graph's mirror, in creation order
  std::vector<uint8_t> zero(cnt, 0), oct1(cnt), oct2(cnt), st1(cnt), st2(cnt);
  std::vector<int32_t> ref(cnt, kf1_slot), slot2(cnt);
  std::vector<uint16_t> idx1(cnt), idx2(cnt);
  for (size_t j = 0; j < cnt; j++) {
    const int k = created_k[j], i1 = created_i1[j];
    if (k < 0 || k >= K || i1 < 0 || i1 >= n1 || created_i2[j] != match12[(size_t)k * (size_t)n1 + (size_t)i1])
      return fail(ORBFE_ERR_HIP, fn + "the device returned an impossible pair");
    const int i2 = created_i2[j];
    const orbfe_frame* F2 = kf2[k];
    slot2[j] = kf2_slot[k];
    idx1[j] = (uint16_t)i1; idx2[j] = (uint16_t)i2;
    oct1[j] = (uint8_t)kf1->hoct[(size_t)i1]; oct2[j] = (uint8_t)F2->hoct[(size_t)i2];
    st1[j] = kf1->hstereo.empty() ? 0 : kf1->hstereo[(size_t)i1];  // the frames' own mvuRight >= 0
    st2[j] = F2->hstereo.empty() ? 0 : F2->hstereo[(size_t)i2];
  }
  bool full = false;
  const char* e = h.set_points(created, new_slot, zero.data(), ref.data());                                                   // MapPoint(x3D, mpCurrentKeyFrame, mpMap)
  if (!e) e = h.add_observations(created, new_slot, ref.data(), idx1.data(), oct1.data(), st1.data(), &full);                // AddObservation(mpCurrentKeyFrame, idx1)
  if (!e && !full) e = h.add_observations(created, new_slot, slot2.data(), idx2.data(), oct2.data(), st2.data(), &full);     // AddObservation(pKF2, idx2)
  if (!e && !full && h.kfRowWidth) e = h.assign_keyframe_points(created, ref.data(), idx1.data(), new_slot);                 // mpCurrentKeyFrame->AddMapPoint
  if (!e && !full && h.kfRowWidth) e = h.assign_keyframe_points(created, slot2.data(), idx2.data(), new_slot);               // pKF2->AddMapPoint
  // check_new_pair_points() accepted them before the launch: a refusal here means the two lists have parted
  if (e || full) return fail(ORBFE_ERR_HIP, fn + "the graph's mirror refused points its own check accepted: " + (e ? e : "a row is full"));
  return ORBFE_OK;
}
