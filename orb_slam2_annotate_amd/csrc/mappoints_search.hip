// mappoints_search.hip -- C-ABI entry points that project or search the device-resident map points (include/orbfe.h:
// orbfe_project_*, orbfe_search_local_points, orbfe_search_*_mappoints*, orbfe_fuse_mappoints), and the four producers
// (window_call.h: Producer) whose prologue kernels (k_project.hip) write the window search's queries from the table.  The
// table is reached through MapPointsLock (host_internal.h), the search machinery through window_call.h.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "frame.h"
#include "host_internal.h"
#include "mappoints_host.h"
#include "match_kernels.h"
#include "obsgraph_kernels.h"
#include "window_call.h"

using namespace orbfe;

namespace {

// up() into a kernel's argument block, whose input pointers are to const
template <typename T>
hipError_t up_arg(Arena* a, const T** d, const T* h, size_t n) {
  T* p = nullptr;
  TRY(up(a, &p, h, n));
  *d = p;
  return hipSuccess;
}

// the slice of a producer's query arrays that starts at window o; its descriptors start at row descRow
QueryOut slice(QueryOut q, size_t o, size_t descRow) {
  q.x += o; q.y += o; q.r += o; q.minLevel += o; q.maxLevel += o; q.active += o;
  if (q.ur) q.ur += o;
  if (q.obs) q.obs += o;
  if (q.desc) q.desc += descRow * 32;
  return q;
}

// Each producer: the caller's operands on the host, and `d`, the kernel's argument block, which upload() fills with where
// they are on the device.  launch() adds where the machinery carved the queries.

// Frame::isInFrustum + the windows of SearchByProjection(Frame&, vector<MapPoint*>&, th) (k_project_frustum): one part
struct FrustumProducer final : Producer {
  MapPointsDevice table{};
  int n = 0;
  const int32_t* slot = nullptr;  // [n]
  const uint8_t* skip = nullptr;  // [n] or NULL
  orbfe_camera_pose pose{};
  float limit = 0.0f, th = 1.0f;
  const float* scale = nullptr;  // [nLevels] mvScaleFactors (a search)
  int nLevels = 0;
  ProjectArgs d{};
  const char* accepts(bool best, int mode) const override {
    return !best && mode == CLAIM_RATIO ? nullptr : "a frustum producer needs a CLAIM_RATIO job";
  }
  int parts() const override { return 1; }
  int queries(int) const override { return n; }
  size_t total() const override { return (size_t)n; }
  bool with_obs() const override { return true; }
  bool with_ur(bool stereo) const override { return stereo; }
  hipError_t upload(Arena* a) override {
    d = ProjectArgs{};
    d.table = table; d.n = n; d.cam = pose; d.limit = limit; d.th = th;
    TRY(up_arg(a, &d.slot, slot, (size_t)n));
    if (skip) TRY(up_arg(a, &d.skip, skip, (size_t)n));
    if (scale) TRY(up_arg(a, &d.scale, scale, (size_t)nLevels));
    return hipSuccess;
  }
  hipError_t launch(hipStream_t s) override {
    d.q = q;
    launch_project_frustum(s, d);
    return hipGetLastError();
  }
  QueryOut part_queries(int) const override { return q; }
  void project_to(void* const* d4, uint8_t* flags) override {  // orbfe_project_in_frustum's order
    d.level = (int32_t*)d4[0]; d.viewCos = (float*)d4[1]; d.projX = (float*)d4[2]; d.projY = (float*)d4[3];
    d.projXr = (float*)d4[4]; d.invZ = (float*)d4[5]; d.dist = (float*)d4[6]; d.inView = flags;
  }
};

// The prologue of ORBmatcher::Fuse for n points against K key-frame poses (k_project_fuse): part k is pose k, every array is
// [k * n + i], and the K parts share one gather of the descriptors
struct FuseProducer final : Producer {
  MapPointsDevice table{};
  const ObsGraphDevice* graph = nullptr;    // NULL: no IsInKeyFrame test
  const int32_t* slot = nullptr;            // [n]
  const uint8_t* skip = nullptr;            // [K * n] or NULL
  const orbfe_camera_pose* pose = nullptr;  // [K]
  const int32_t* kfSlot = nullptr;          // [K] (with graph)
  int n = 0, K = 0;
  const float* scale = nullptr;        // [nLevels] mvScaleFactors (a search)
  const float* hInvSigma2 = nullptr;   // [nLevels] mvInvLevelSigma2 (gate)
  int nLevels = 0;
  float th = 3.0f;
  bool gate = false;
  FuseArgs d{};
  // (BEST jobs: Fuse; CLAIM_BEST: the Sim3 SearchByProjection, whose prologue is Fuse's)
  const char* accepts(bool best, int mode) const override {
    return best || mode == CLAIM_BEST ? nullptr : "a fuse producer needs BEST or CLAIM_BEST jobs";
  }
  int parts() const override { return K; }
  int queries(int) const override { return n; }
  size_t total() const override { return (size_t)K * n; }
  size_t desc_rows() const override { return (size_t)n; }
  bool with_ur(bool) const override { return gate; }  // (the chi-square gate reads it, whatever the frame)
  hipError_t upload(Arena* a) override {
    d = FuseArgs{};
    d.table = table; d.n = n; d.K = K; d.th = th;
    if (graph) { d.rows = graph->rows; d.meta = graph->meta; d.rowWidth = graph->rowWidth; d.pointCap = graph->pointCap; }
    TRY(up_arg(a, &d.slot, slot, (size_t)n));
    if (skip) TRY(up_arg(a, &d.skip, skip, total()));
    TRY(up_arg(a, &d.pose, pose, (size_t)K));
    if (graph) TRY(up_arg(a, &d.kfSlot, kfSlot, (size_t)K));
    if (scale) TRY(up_arg(a, &d.scale, scale, (size_t)nLevels));
    invSigma2 = nullptr;
    if (gate) TRY(up(a, &invSigma2, hInvSigma2, (size_t)nLevels));
    return hipSuccess;
  }
  hipError_t launch(hipStream_t s) override {
    d.q = q;
    launch_project_fuse(s, d);
    return hipGetLastError();
  }
  QueryOut part_queries(int k) const override { return slice(q, (size_t)k * n, 0); }
  void project_to(void* const* d4, uint8_t* flags) override {  // orbfe_project_fuse's order
    d.u = (float*)d4[0]; d.v = (float*)d4[1]; d.ur = (float*)d4[2]; d.level = (int32_t*)d4[3]; d.dist = (float*)d4[4];
    d.valid = flags;
  }
};

// The prologue of the last-frame (form 0) or key-frame (form 1) SearchByProjection for K jobs over concatenated lists
// (k_project_track): part k is list k, every array is by position in the concatenation
struct TrackProducer final : Producer {
  MapPointsDevice table{};
  int form = 0, K = 0, mode = 0;
  const int32_t* offsets = nullptr;         // [K + 1]
  const int32_t* slot = nullptr;            // [offsets[K]]
  const uint8_t* skip = nullptr;            // [offsets[K]] or NULL
  const int32_t* lastOctave = nullptr;      // [offsets[K]] (form 0)
  const orbfe_camera_pose* pose = nullptr;  // [K]
  const float* th = nullptr;                // [K] (a search, or form 0's radius)
  const float* scale = nullptr;             // [nLevels] mvScaleFactors (likewise)
  int nLevels = 0;
  TrackArgs d{};
  const char* accepts(bool best, int claimMode) const override {
    return !best && claimMode == CLAIM_BEST ? nullptr : "a track producer needs CLAIM_BEST jobs";
  }
  int parts() const override { return K; }
  int queries(int k) const override { return offsets[k + 1] - offsets[k]; }
  size_t total() const override { return (size_t)offsets[K]; }
  bool with_obs() const override { return form == 0; }
  bool with_ur(bool stereo) const override { return form == 0 && stereo; }
  hipError_t upload(Arena* a) override {
    d = TrackArgs{};
    d.table = table; d.form = form; d.K = K; d.mode = mode;
    TRY(up_arg(a, &d.offsets, offsets, (size_t)K + 1));
    TRY(up_arg(a, &d.slot, slot, total()));
    if (skip) TRY(up_arg(a, &d.skip, skip, total()));
    if (form == 0) TRY(up_arg(a, &d.lastOctave, lastOctave, total()));
    TRY(up_arg(a, &d.pose, pose, (size_t)K));
    if (th) TRY(up_arg(a, &d.th, th, (size_t)K));
    if (scale) TRY(up_arg(a, &d.scale, scale, (size_t)nLevels));
    return hipSuccess;
  }
  hipError_t launch(hipStream_t s) override {
    int longest = 0;
    for (int k = 0; k < K; k++) longest = queries(k) > longest ? queries(k) : longest;
    d.q = q;
    launch_project_track(s, d, longest);
    return hipGetLastError();
  }
  QueryOut part_queries(int k) const override { return slice(q, (size_t)offsets[k], (size_t)offsets[k]); }
  // orbfe_project_last_frame's order (u, v, inv_z, ur, radius) or orbfe_project_keyframe's (u, v, inv_z, level, dist)
  void project_to(void* const* d4, uint8_t* flags) override {
    d.u = (float*)d4[0]; d.v = (float*)d4[1]; d.invZ = (float*)d4[2]; d.valid = flags;
    if (form == 0) { d.ur = (float*)d4[3]; d.radius = (float*)d4[4]; }
    else { d.level = (int32_t*)d4[3]; d.dist = (float*)d4[4]; }
  }
};

// The prologue of SearchBySim3 for nLegs legs (k_project_sim3): part l is leg l.  slot[] holds every source list once (KF1's,
// then the candidates'); the outputs and skip[] are by OUTPUT position (a leg's span says where both start), so K legs may
// read one list, and a leg's descriptors lie where its slots do.
static_assert(kSim3MaxLegs == kSim3MaxLegRecords, "the kernel's leg limit is the one sim3_check_legs enforces");
struct Sim3Producer final : Producer {
  MapPointsDevice table{};
  int nLegs = 0;
  const Sim3Span* span = nullptr;        // [nLegs]
  const orbfe_sim3_leg* leg = nullptr;   // [nLegs]
  const int32_t* slot = nullptr; size_t nSlot = 0;
  const uint8_t* skip = nullptr; size_t nOut = 0;  // [nOut] or NULL
  const float* scale = nullptr;          // [nScale] level table(s) (a search)
  int nScale = 0, nLevels = 0;
  float th = 0.0f;
  // vbAlreadyMatched2 from the observation rows (graph != NULL): a scatter into skip[already2Off ..] ahead of the prologue
  const ObsGraphDevice* graph = nullptr;
  const int32_t *matched = nullptr, *kfSlot = nullptr, *offsets2 = nullptr;
  int K = 0, n1 = 0;
  size_t already2Off = 0;
  Sim3Args d{};
  uint8_t* dSkip = nullptr;  // d.skip, writable for the scatter
  const int32_t *dMatched = nullptr, *dKfSlot = nullptr, *dOffsets2 = nullptr;
  const char* accepts(bool best, int) const override { return best ? nullptr : "a sim3 producer needs BEST jobs"; }
  int parts() const override { return nLegs; }
  int queries(int l) const override { return span[l].n; }
  size_t total() const override { return nOut; }
  size_t desc_rows() const override { return nSlot; }
  bool with_ur(bool) const override { return false; }
  hipError_t upload(Arena* a) override {
    d = Sim3Args{};
    dSkip = nullptr;
    d.table = table; d.nLegs = nLegs; d.nLevels = nLevels; d.th = th;
    TRY(up_arg(a, &d.span, span, (size_t)nLegs));
    TRY(up_arg(a, &d.leg, leg, (size_t)nLegs));
    TRY(up_arg(a, &d.slot, slot, nSlot));
    if (skip) TRY(up(a, &dSkip, skip, nOut));
    d.skip = dSkip;
    if (scale) TRY(up_arg(a, &d.scale, scale, (size_t)nScale));
    if (graph) {
      TRY(up_arg(a, &dMatched, matched, (size_t)K * n1));
      TRY(up_arg(a, &dKfSlot, kfSlot, (size_t)K));
      TRY(up_arg(a, &dOffsets2, offsets2, (size_t)K + 1));
    }
    return hipSuccess;
  }
  hipError_t launch(hipStream_t s) override {
    if (graph) {
      launch_sim3_already(s, graph->rows, graph->meta, graph->rowWidth, graph->pointCap, K, n1, dMatched, dKfSlot, dOffsets2,
                          dSkip + already2Off);
      TRY(hipGetLastError());
    }
    int longest = 0;
    for (int l = 0; l < nLegs; l++) longest = span[l].n > longest ? span[l].n : longest;
    d.q = q;
    launch_project_sim3(s, d, longest);
    return hipGetLastError();
  }
  QueryOut part_queries(int l) const override { return slice(q, (size_t)span[l].outOff, (size_t)span[l].slotOff); }
  void project_to(void* const* d4, uint8_t* flags) override {  // orbfe_project_sim3's order
    d.u = (float*)d4[0]; d.v = (float*)d4[1]; d.level = (int32_t*)d4[2]; d.dist = (float*)d4[3]; d.valid = flags;
  }
};

}  // namespace

// ---------------------------------------------------------------------------------------------
// Frame::isInFrustum and Tracking::SearchLocalPoints
// ---------------------------------------------------------------------------------------------
extern "C" int orbfe_project_in_frustum(orbfe_mappoints* mp, int n, const int32_t* slot, const uint8_t* skip,
                                        const orbfe_camera_pose* pose, float viewing_cos_limit, uint8_t* in_view, int32_t* level,
                                        float* view_cos, float* proj_x, float* proj_y, float* proj_xr, float* inv_z, float* dist) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "project_in_frustum: NULL table");
  if (const char* e = mappoints_check_slots(orbfe_mappoints_capacity(mp), n, slot)) return fail(ORBFE_ERR_INVALID, std::string("project_in_frustum: ") + e);
  if (!pose_ok(pose)) return fail(ORBFE_ERR_INVALID, "project_in_frustum: bad pose (n_levels must be 1 .. 64)");
  if (n == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  FrustumProducer P;
  P.table = *lock.table; P.n = n; P.slot = slot; P.skip = skip; P.pose = *pose; P.limit = viewing_cos_limit;
  void* const out4[] = {level, view_cos, proj_x, proj_y, proj_xr, inv_z, dist};
  return producer_run(lock.device, P, 7, out4, in_view);
}

extern "C" int orbfe_search_local_points(orbfe_mappoints* mp, int n, const int32_t* slot, const uint8_t* skip,
                                         const orbfe_camera_pose* pose, float viewing_cos_limit, const orbfe_frame_view* F,
                                         const float* scale_factors, int n_levels, const uint8_t* blocked, float th, float nnratio,
                                         int32_t* match, int32_t* n_matches, uint8_t* in_view) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "search_local_points: NULL table");
  if (const char* e = mappoints_check_slots(orbfe_mappoints_capacity(mp), n, slot)) return fail(ORBFE_ERR_INVALID, std::string("search_local_points: ") + e);
  F = canon(F);
  if (!frame_ok(F) || !scale_factors || n_levels <= 0 || !pose_ok(pose) || pose->n_levels > n_levels || !n_matches ||
      (F->n > 0 && (!match || !F->desc)))
    return fail(ORBFE_ERR_INVALID, "search_local_points: bad argument");
  for (int i = 0; i < F->n; i++) match[i] = -1;
  *n_matches = 0;
  if (n == 0) return ORBFE_OK;
  if (F->n == 0) {  // nothing to search: the flags alone
    return in_view ? orbfe_project_in_frustum(mp, n, slot, skip, pose, viewing_cos_limit, in_view, nullptr, nullptr, nullptr, nullptr, nullptr,
                                              nullptr, nullptr)
                   : ORBFE_OK;
  }
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  FrustumProducer P;
  P.table = *lock.table; P.n = n; P.slot = slot; P.skip = skip; P.pose = *pose; P.limit = viewing_cos_limit; P.th = th;
  P.scale = scale_factors; P.nLevels = n_levels; P.flagsOut = in_view;
  ClaimSpec C;
  C.mode = CLAIM_RATIO; C.maxDist = 100 /* TH_HIGH */; C.nnratio = nnratio;
  C.blocked = blocked;
  C.match = match; C.nMatches = n_matches;
  WindowJob job;
  job.f = F; job.nq = n;
  job.claim = &C;
  job.producer = &P;
  return window_search_multi(lock.device, &job, 1, 32);
}

// ---------------------------------------------------------------------------------------------
// The two tracking-thread searches that walk a frame's own map points: k_project_track writes the windows the host-array
// calls (matcher.hip) build from the caller's projection, and the same window search and claim launches follow.
// ---------------------------------------------------------------------------------------------
extern "C" int orbfe_project_last_frame(orbfe_mappoints* mp, int n, const int32_t* slot, const uint8_t* skip,
                                        const int32_t* last_octave, const orbfe_camera_pose* pose, const float* scale_factors,
                                        int n_levels, float th, int mode, uint8_t* valid, float* u, float* v, float* inv_z, float* ur,
                                        float* radius) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "project_last_frame: NULL table");
  if (!scale_factors || n_levels <= 0 || mode < 0 || mode > 2) return fail(ORBFE_ERR_INVALID, "project_last_frame: bad argument");
  const int32_t offsets[2] = {0, n};
  if (const char* e = track_check_operands(orbfe_mappoints_capacity(mp), 1, offsets, slot, true, last_octave, pose, n_levels))
    return fail(ORBFE_ERR_INVALID, std::string("project_last_frame: ") + e);
  if (n == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  TrackProducer P;
  P.table = *lock.table; P.form = 0; P.K = 1; P.mode = mode; P.offsets = offsets; P.slot = slot; P.skip = skip;
  P.lastOctave = last_octave; P.pose = pose; P.th = &th; P.scale = scale_factors; P.nLevels = n_levels;
  void* const out4[] = {u, v, inv_z, ur, radius};
  return producer_run(lock.device, P, 5, out4, valid);
}

extern "C" int orbfe_search_last_frame_mappoints(orbfe_mappoints* mp, int n, const int32_t* slot, const uint8_t* skip,
                                                 const int32_t* last_octave, const float* last_angle, const orbfe_camera_pose* pose,
                                                 const orbfe_frame_view* Cur, const float* scale_factors, int n_levels,
                                                 const uint8_t* blocked, int mode, float th, int check_orientation,
                                                 int32_t* match_cur, int32_t* n_matches, uint8_t* valid_out) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "search_last_frame_mappoints: NULL table");
  const int32_t offsets[2] = {0, n};
  if (const char* e = track_check_operands(orbfe_mappoints_capacity(mp), 1, offsets, slot, true, last_octave, pose, n_levels))
    return fail(ORBFE_ERR_INVALID, std::string("search_last_frame_mappoints: ") + e);
  Cur = canon(Cur);
  if (!frame_ok(Cur) || !scale_factors || n_levels <= 0 || !n_matches || mode < 0 || mode > 2 ||
      (Cur->n > 0 && (!match_cur || !Cur->desc)) || (check_orientation && Cur->n > 0 && !Cur->angle) ||
      (check_orientation && n > 0 && !last_angle))
    return fail(ORBFE_ERR_INVALID, "search_last_frame_mappoints: bad argument");
  for (int i = 0; i < Cur->n; i++) match_cur[i] = -1;
  *n_matches = 0;
  if (n == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  TrackProducer P;
  P.table = *lock.table; P.form = 0; P.K = 1; P.mode = mode; P.offsets = offsets; P.slot = slot; P.skip = skip;
  P.lastOctave = last_octave; P.pose = pose; P.th = &th; P.scale = scale_factors; P.nLevels = n_levels; P.flagsOut = valid_out;
  if (Cur->n == 0) {  // nothing to search: the flags alone
    void* const none[5] = {};
    return valid_out ? producer_run(lock.device, P, 5, none, valid_out) : ORBFE_OK;
  }
  ClaimSpec C = last_frame_claim(blocked, nullptr, last_angle, check_orientation, match_cur, n_matches);
  WindowJob job;
  job.f = Cur; job.nq = n;
  job.claim = &C;
  job.producer = &P; job.part = 0;
  return window_search_multi(lock.device, &job, 1, 32);
}

extern "C" int orbfe_project_keyframe(orbfe_mappoints* mp, int n_candidates, const int32_t* offsets, const int32_t* slot,
                                      const uint8_t* skip, const orbfe_camera_pose* pose, uint8_t* valid, float* u, float* v,
                                      float* inv_z, int32_t* level, float* dist) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "project_keyframe: NULL table");
  if (const char* e = track_check_operands(orbfe_mappoints_capacity(mp), n_candidates, offsets, slot, false, nullptr, pose, 0))
    return fail(ORBFE_ERR_INVALID, std::string("project_keyframe: ") + e);
  if (n_candidates == 0 || offsets[n_candidates] == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  TrackProducer P;
  P.table = *lock.table; P.form = 1; P.K = n_candidates; P.offsets = offsets; P.slot = slot; P.skip = skip; P.pose = pose;
  void* const out4[] = {u, v, inv_z, level, dist};
  return producer_run(lock.device, P, 5, out4, valid);
}

extern "C" int orbfe_search_keyframe_mappoints_multi(orbfe_mappoints* mp, const orbfe_frame_view* Cur, const float* scale_factors,
                                                     int n_levels, int n_candidates, const int32_t* offsets, const int32_t* slot,
                                                     const uint8_t* skip, const float* kf_angle, const orbfe_camera_pose* pose,
                                                     const uint8_t* const* blocked, const float* th, const int32_t* orb_dist,
                                                     int check_orientation, int32_t* match_cur, int32_t* n_matches) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "search_keyframe_mappoints_multi: NULL table");
  const int K = n_candidates;
  if (const char* e = track_check_operands(orbfe_mappoints_capacity(mp), K, offsets, slot, false, nullptr, pose, n_levels))
    return fail(ORBFE_ERR_INVALID, std::string("search_keyframe_mappoints_multi: ") + e);
  Cur = canon(Cur);
  if (!frame_ok(Cur) || !scale_factors || n_levels <= 0 || (K > 0 && (!th || !orb_dist || !n_matches)) ||
      (Cur->n > 0 && K > 0 && (!match_cur || !Cur->desc)) || (check_orientation && Cur->n > 0 && !Cur->angle) ||
      (check_orientation && K > 0 && offsets[K] > 0 && !kf_angle))
    return fail(ORBFE_ERR_INVALID, "search_keyframe_mappoints_multi: bad argument");
  if (K == 0) return ORBFE_OK;
  for (size_t i = 0; i < (size_t)K * Cur->n; i++) match_cur[i] = -1;
  for (int k = 0; k < K; k++) n_matches[k] = 0;
  if (offsets[K] == 0 || Cur->n == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  TrackProducer P;
  P.table = *lock.table; P.form = 1; P.K = K; P.offsets = offsets; P.slot = slot; P.skip = skip; P.pose = pose; P.th = th;
  P.scale = scale_factors; P.nLevels = n_levels;
  std::vector<ClaimSpec> claims((size_t)K);
  std::vector<WindowJob> wj;
  for (int k = 0; k < K; k++) {
    if (offsets[k + 1] == offsets[k]) continue;  // an empty candidate: its matches stay -1
    claims[k] = keyframe_claim(blocked ? blocked[k] : nullptr, check_orientation ? kf_angle + offsets[k] : nullptr, orb_dist[k],
                               check_orientation, match_cur + (size_t)k * Cur->n, &n_matches[k]);
    WindowJob job;
    job.f = Cur; job.nq = offsets[k + 1] - offsets[k];
    job.claim = &claims[k];
    job.producer = &P; job.part = k;
    wj.push_back(job);
  }
  // one claim workgroup per candidate behind the K window searches: one upload, one launch group, one download
  return window_search_multi(lock.device, wj.data(), (int)wj.size(), 32);
}

// ---------------------------------------------------------------------------------------------
// ORBmatcher::Fuse
// ---------------------------------------------------------------------------------------------
extern "C" int orbfe_project_fuse(orbfe_mappoints* mp, orbfe_obsgraph* g, int n, const int32_t* slot, int n_keyframes,
                                  const int32_t* kf_slot, const orbfe_camera_pose* pose, const uint8_t* skip, uint8_t* valid, float* u,
                                  float* v, float* ur, int32_t* level, float* dist) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "project_fuse: NULL table");
  ObsGraphLock glock(g);  // the graph's serialisation first, then the table's: the order of orbfe_obsgraph_*_mappoints
  if (g && mappoints_device(mp) != glock.device) return fail(ORBFE_ERR_INVALID, "project_fuse: the graph and the map-point table are on different devices");
  if (const char* e = fuse_check_operands(orbfe_mappoints_capacity(mp), n, slot, n_keyframes, kf_slot, g != nullptr, glock.kfCap, pose, 0))
    return fail(ORBFE_ERR_INVALID, std::string("project_fuse: ") + e);
  if (n == 0 || n_keyframes == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  if (int rc = glock.table_ready()) return rc;
  FuseProducer P;
  P.table = *lock.table; P.graph = glock.graph; P.slot = slot; P.skip = skip; P.pose = pose; P.kfSlot = kf_slot; P.n = n; P.K = n_keyframes;
  void* const out4[] = {u, v, ur, level, dist};
  return producer_run(lock.device, P, 5, out4, valid);
}

extern "C" int orbfe_fuse_mappoints(orbfe_mappoints* mp, orbfe_obsgraph* g, int n, const int32_t* slot, int n_keyframes,
                                    const orbfe_frame_view* const* KF, const int32_t* kf_slot, const orbfe_camera_pose* pose,
                                    const uint8_t* skip, const float* scale_factors, const float* inv_level_sigma2, int n_levels,
                                    float th, int chi2_gate, int32_t* best_idx, uint8_t* projected) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "fuse_mappoints: NULL table");
  if (!scale_factors || n_levels <= 0 || (chi2_gate && !inv_level_sigma2) || (n_keyframes > 0 && !KF) ||
      (n_keyframes > 0 && n > 0 && !best_idx))
    return fail(ORBFE_ERR_INVALID, "fuse_mappoints: bad argument");
  ObsGraphLock glock(g);  // the graph's serialisation first, then the table's: the order of orbfe_obsgraph_*_mappoints
  if (g && mappoints_device(mp) != glock.device) return fail(ORBFE_ERR_INVALID, "fuse_mappoints: the graph and the map-point table are on different devices");
  if (const char* e = fuse_check_operands(orbfe_mappoints_capacity(mp), n, slot, n_keyframes, kf_slot, g != nullptr, glock.kfCap, pose, n_levels))
    return fail(ORBFE_ERR_INVALID, std::string("fuse_mappoints: ") + e);
  std::vector<const orbfe_frame_view*> views;
  for (int k = 0; k < n_keyframes; k++) {  // (orbfe_fuse_search_multi's checks of its key frames)
    const orbfe_frame_view* f = canon(KF[k]);
    if (!frame_ok(f) || (f->n > 0 && !f->desc)) return fail(ORBFE_ERR_INVALID, "fuse_mappoints: bad key frame view");
    for (int i = 0; i < f->n; i++)
      if (chi2_gate && (f->octave[i] < 0 || f->octave[i] >= n_levels))
        return fail(ORBFE_ERR_INVALID, "fuse_mappoints: keypoint octave outside the pyramid");
    views.push_back(f);
  }
  if (n == 0 || n_keyframes == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  if (int rc = glock.table_ready()) return rc;
  for (size_t i = 0; i < (size_t)n_keyframes * n; i++) best_idx[i] = -1;
  FuseProducer P;
  P.table = *lock.table; P.graph = glock.graph; P.slot = slot; P.skip = skip; P.pose = pose; P.kfSlot = kf_slot; P.n = n; P.K = n_keyframes;
  std::vector<WindowJob> wj;
  for (int k = 0; k < n_keyframes; k++) {
    if (views[(size_t)k]->n == 0) continue;  // nothing to search: every best_idx of the key frame stays -1
    WindowJob w;
    w.f = views[(size_t)k]; w.nq = n;
    w.bestOut = best_idx + (size_t)k * n;
    w.gate = chi2_gate ? 1 : 0; w.nLevels = n_levels; w.maxDist = 50 /* TH_LOW */;
    w.producer = &P; w.part = k;
    wj.push_back(w);
  }
  if (wj.empty()) {  // K empty key frames: the prologue alone, if the caller asked for it
    void* const none[5] = {};
    return projected ? producer_run(lock.device, P, 5, none, projected) : ORBFE_OK;
  }
  P.scale = scale_factors; P.hInvSigma2 = inv_level_sigma2; P.nLevels = n_levels; P.th = th; P.gate = chi2_gate != 0;
  P.flagsOut = projected;
  return window_search_multi(lock.device, wj.data(), (int)wj.size(), 8);
}

// ---------------------------------------------------------------------------------------------
// ORBmatcher::SearchBySim3 and the Sim3 SearchByProjection (LoopClosing::ComputeSim3)
// ---------------------------------------------------------------------------------------------
extern "C" int orbfe_project_sim3(orbfe_mappoints* mp, int n_legs, const int32_t* offsets, const int32_t* slot, const uint8_t* skip,
                                  const orbfe_sim3_leg* legs, uint8_t* valid, float* u, float* v, int32_t* level, float* dist) {
  if (!mp) return fail(ORBFE_ERR_INVALID, "project_sim3: NULL table");
  if (const char* e = sim3_check_legs(orbfe_mappoints_capacity(mp), n_legs, offsets, slot, legs, 0))
    return fail(ORBFE_ERR_INVALID, std::string("project_sim3: ") + e);
  if (n_legs == 0 || offsets[n_legs] == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  std::vector<Sim3Span> span((size_t)n_legs);
  for (int l = 0; l < n_legs; l++) span[(size_t)l] = Sim3Span{offsets[l], offsets[l + 1] - offsets[l], offsets[l], 0};
  Sim3Producer P;
  P.table = *lock.table; P.nLegs = n_legs; P.span = span.data(); P.leg = legs; P.slot = slot; P.nSlot = (size_t)offsets[n_legs];
  P.skip = skip; P.nOut = P.nSlot;
  void* const out4[] = {u, v, level, dist};
  return producer_run(lock.device, P, 4, out4, valid);
}

// SearchBySim3 for K candidates of one key frame: legs 2k (KF1 -> KF2_k) and 2k + 1 (KF2_k -> KF1) of ONE prologue launch, 2K
// BEST window jobs of one search launch, the agreement check (:1461-1474) over the one download
extern "C" int orbfe_search_by_sim3_mappoints_multi(orbfe_mappoints* mp, orbfe_obsgraph* g, const orbfe_frame_view* KF1,
                                                    const int32_t* slot1, int n_candidates, const orbfe_frame_view* const* KF2,
                                                    const int32_t* offsets2, const int32_t* slot2, const orbfe_sim3_leg* legs12,
                                                    const orbfe_sim3_leg* legs21, const int32_t* matched12_in, const int32_t* kf2_slot,
                                                    const uint8_t* already2, const float* scale_factors1, const float* scale_factors2,
                                                    int n_levels, float th, int32_t* match12, int32_t* n_found) {
  const char* who = "search_by_sim3_mappoints_multi: ";
  if (!mp) return fail(ORBFE_ERR_INVALID, std::string(who) + "NULL table");
  const int K = n_candidates;
  KF1 = canon(KF1);
  if (!frame_ok(KF1) || (KF1->n > 0 && !KF1->desc)) return fail(ORBFE_ERR_INVALID, std::string(who) + "bad key frame view");
  const int N1 = KF1->n;
  const bool withGraph = g != nullptr && kf2_slot != nullptr;
  ObsGraphLock glock(withGraph ? g : nullptr);  // the graph's serialisation first, then the table's
  if (withGraph && mappoints_device(mp) != glock.device)
    return fail(ORBFE_ERR_INVALID, std::string(who) + "the graph and the map-point table are on different devices");
  if (const char* e = sim3_check_search(orbfe_mappoints_capacity(mp), N1, slot1, K, offsets2, slot2, legs12, legs21, matched12_in, kf2_slot,
                                        withGraph, glock.kfCap, n_levels))
    return fail(ORBFE_ERR_INVALID, std::string(who) + e);
  if (K == 0) return ORBFE_OK;
  if (!KF2 || !scale_factors1 || !scale_factors2 || !n_found || (N1 > 0 && !match12))
    return fail(ORBFE_ERR_INVALID, std::string(who) + "NULL argument");
  std::vector<const orbfe_frame_view*> views((size_t)K);
  for (int k = 0; k < K; k++) {
    const orbfe_frame_view* f = canon(KF2[k]);
    if (!frame_ok(f) || (f->n > 0 && !f->desc)) return fail(ORBFE_ERR_INVALID, std::string(who) + "bad key frame view");
    if (f->n != offsets2[k + 1] - offsets2[k]) return fail(ORBFE_ERR_INVALID, std::string(who) + "slot2 does not hold KF2->n entries per candidate");
    views[(size_t)k] = f;
  }
  for (size_t i = 0; i < (size_t)K * N1; i++) match12[i] = -1;
  for (int k = 0; k < K; k++) n_found[k] = 0;
  const size_t total2 = (size_t)offsets2[K], out2 = (size_t)K * N1;
  if (N1 == 0 || total2 == 0) return ORBFE_OK;  // (a direction without a point finds nothing, so no pair can agree)
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  if (int rc = glock.table_ready()) return rc;
  // what travels: KF1's list once, then the candidates'; the masks by output position (K x N1, then the candidates')
  std::vector<int32_t> slot((size_t)N1 + total2);
  std::memcpy(slot.data(), slot1, (size_t)N1 * 4);
  std::memcpy(slot.data() + N1, slot2, total2 * 4);
  std::vector<uint8_t> skip(out2 + total2, 0);
  if (matched12_in)
    for (size_t i = 0; i < out2; i++) skip[i] = matched12_in[i] >= 0;
  if (already2)
    for (size_t i = 0; i < total2; i++) skip[out2 + i] = already2[i] != 0;
  std::vector<Sim3Span> span((size_t)2 * K);
  std::vector<orbfe_sim3_leg> leg((size_t)2 * K);
  for (int k = 0; k < K; k++) {
    span[2 * (size_t)k] = Sim3Span{0, N1, (int32_t)((size_t)k * N1), (k == 0 ? 1 : 0) | 2};  // KF2_k's level table is the second
    span[2 * (size_t)k + 1] = Sim3Span{N1 + offsets2[k], offsets2[k + 1] - offsets2[k], (int32_t)(out2 + (size_t)offsets2[k]), 1};
    leg[2 * (size_t)k] = legs12[k];
    leg[2 * (size_t)k + 1] = legs21[k];
  }
  std::vector<float> scale((size_t)2 * n_levels);
  std::memcpy(scale.data(), scale_factors1, (size_t)n_levels * 4);
  std::memcpy(scale.data() + n_levels, scale_factors2, (size_t)n_levels * 4);
  Sim3Producer P;
  P.table = *lock.table; P.nLegs = 2 * K; P.span = span.data(); P.leg = leg.data(); P.slot = slot.data(); P.nSlot = slot.size();
  P.skip = skip.data(); P.nOut = skip.size(); P.scale = scale.data(); P.nScale = 2 * n_levels; P.nLevels = n_levels; P.th = th;
  if (withGraph && matched12_in) {
    P.graph = glock.graph; P.matched = matched12_in; P.kfSlot = kf2_slot; P.offsets2 = offsets2; P.K = K; P.n1 = N1; P.already2Off = out2;
  }
  std::vector<int32_t> m2(total2, -1);  // vnMatch2 of every candidate; match12 holds vnMatch1 until the agreement check
  std::vector<WindowJob> wj;
  for (int k = 0; k < K; k++) {
    const int n2 = views[(size_t)k]->n;
    if (n2 == 0) continue;  // nothing to search in either direction
    WindowJob a, b;
    a.f = views[(size_t)k]; a.nq = N1; a.bestOut = match12 + (size_t)k * N1; a.maxDist = 100 /* TH_HIGH */; a.nLevels = n_levels;
    a.producer = &P; a.part = 2 * k;
    b.f = KF1; b.nq = n2; b.bestOut = m2.data() + offsets2[k]; b.maxDist = 100; b.nLevels = n_levels;
    b.producer = &P; b.part = 2 * k + 1;
    wj.push_back(a);
    wj.push_back(b);
  }
  if (int rc = window_search_multi(lock.device, wj.data(), (int)wj.size(), 8)) return rc;
  for (int k = 0; k < K; k++) {
    int32_t* m1 = match12 + (size_t)k * N1;
    const int32_t* mk = m2.data() + offsets2[k];
    int nFound = 0;
    for (int i1 = 0; i1 < N1; i1++) {
      const int idx2 = m1[i1];
      if (idx2 >= 0 && mk[idx2] == i1) nFound++; else m1[i1] = -1;
    }
    n_found[k] = nFound;
  }
  return ORBFE_OK;
}

// SearchByProjection(pKF, Scw, vpPoints, vpMatched, th): k_project_fuse at K = 1 without a graph in front of the claim loop
extern "C" int orbfe_search_by_projection_sim3_mappoints(orbfe_mappoints* mp, int n, const int32_t* slot, const uint8_t* skip,
                                                         const orbfe_camera_pose* pose, const orbfe_frame_view* KF,
                                                         const float* scale_factors, int n_levels, const uint8_t* matched, float th,
                                                         int32_t* match, int32_t* n_matches, uint8_t* projected) {
  const char* who = "search_by_projection_sim3_mappoints: ";
  if (!mp) return fail(ORBFE_ERR_INVALID, std::string(who) + "NULL table");
  KF = canon(KF);
  if (!frame_ok(KF) || !scale_factors || n_levels <= 0 || !n_matches || (KF->n > 0 && (!match || !KF->desc)))
    return fail(ORBFE_ERR_INVALID, std::string(who) + "bad argument");
  if (const char* e = fuse_check_operands(orbfe_mappoints_capacity(mp), n, slot, 1, nullptr, false, 0, pose, n_levels))
    return fail(ORBFE_ERR_INVALID, std::string(who) + e);
  for (int i = 0; i < KF->n; i++) match[i] = -1;
  *n_matches = 0;
  if (n == 0) return ORBFE_OK;
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  FuseProducer P;
  P.table = *lock.table; P.slot = slot; P.skip = skip; P.pose = pose; P.n = n; P.K = 1;
  if (KF->n == 0) {  // nothing to search: the flags alone
    void* const none[5] = {};
    return projected ? producer_run(lock.device, P, 5, none, projected) : ORBFE_OK;
  }
  P.scale = scale_factors; P.nLevels = n_levels; P.th = th; P.flagsOut = projected;
  ClaimSpec C;  // claim loop :418-446 on the device
  C.mode = CLAIM_BEST; C.maxDist = 50 /* TH_LOW */;
  C.blocked = matched;
  C.match = match; C.nMatches = n_matches;
  WindowJob job;
  job.f = KF; job.nq = n;
  job.claim = &C;
  job.producer = &P; job.part = 0;
  return window_search_multi(lock.device, &job, 1, 32);
}
