// loopcorrect.hip -- host side of the loop correction (include/orbfe.h: orbfe_correct_loop_*, orbfe_gba_*; kernels:
// k_loopcorrect.hip; host arithmetic: loopcorrect_host.h).  References: LoopClosing::CorrectLoop
// (src/LoopClosing.cc:514-604) and the tail of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:787-852).
//
// The two resident calls are the graph's: they take its serialisation, then the map-point table's, run on the graph's one
// stream and are complete on return.  Every operand is checked before anything is enqueued.  The kf-slot-to-place table
// (orbfe_obsgraph::kfRank) is -1 everywhere between calls: a call writes the listed slots and writes them back; a call
// that fails between the two drops the table, and the next one makes a fresh one.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/orbfe.h"
#include "host_internal.h"
#include "loopcorrect_host.h"
#include "loopcorrect_kernels.h"
#include "obsgraph_handle.h"
#include "obsgraph_host.h"

using namespace orbfe;

namespace {

bool distinct(int n, const int32_t* v) {
  std::vector<int32_t> sorted(v, v + n);
  std::sort(sorted.begin(), sorted.end());
  return std::adjacent_find(sorted.begin(), sorted.end()) == sorted.end();
}

// the rank table on the device, idle; drops it again unless the call reaches its end
struct RankScope {
  orbfe_obsgraph* g;
  bool done = false;
  explicit RankScope(orbfe_obsgraph* g_) : g(g_) {}
  ~RankScope() {
    if (!done) g->kfRank.reset();
  }
  int ready() {
    if (g->kfRank.p) return ORBFE_OK;
    if (int rc = g->kfRank.alloc((size_t)g->h.kfCap)) return rc;
    HIPCHK(hipMemsetAsync(g->kfRank.p, 0xff, (size_t)g->h.kfCap * 4, g->arena.stream));
    return ORBFE_OK;
  }
};

const char* check_tables(orbfe_obsgraph* g, orbfe_mappoints* mp) {
  if (mappoints_device(mp) != g->device) return "the graph and the map-point table are on different devices";
  if (g->h.pointCap > orbfe_mappoints_capacity(mp)) return "the graph has more point slots than the map-point table";
  return nullptr;
}

}  // namespace

extern "C" int orbfe_correct_loop_sim3s(int K, const float* Tiw, const float* Twc_cur, int cur, const double* Scw, double* corrected,
                                        double* noncorrected, float* Tiw_corrected) {
  if (const char* e = correct_loop_sim3s(K, Tiw, Twc_cur, cur, Scw, corrected, noncorrected, Tiw_corrected))
    return obs_invalid("correct_loop_sim3s", e);
  return ORBFE_OK;
}

extern "C" int orbfe_correct_loop_points(int K, const double* corrected, const double* noncorrected, const int32_t* offsets,
                                         const int32_t* point, int n_points, const float* xw, const uint8_t* skip, float* xw_out,
                                         int32_t* corrected_ref) {
  if (const char* e = correct_loop_points(K, corrected, noncorrected, offsets, point, n_points, xw, skip, xw_out, corrected_ref))
    return obs_invalid("correct_loop_points", e);
  return ORBFE_OK;
}

extern "C" int orbfe_gba_propagate_keyframes(int n, int n_origins, const int32_t* origin, const int32_t* child_offsets, const int32_t* child,
                                             const float* Tcw, const float* Twc, const uint8_t* in_gba, const float* Tcw_gba, float* Tcw_new,
                                             uint8_t* reached, uint8_t* visited) {
  if (const char* e = gba_propagate_keyframes(n, n_origins, origin, child_offsets, child, Tcw, Twc, in_gba, Tcw_gba, Tcw_new, reached, visited))
    return obs_invalid("gba_propagate_keyframes", e);
  return ORBFE_OK;
}

extern "C" int orbfe_gba_update_points(int n_points, const float* xw, const uint8_t* bad, const uint8_t* in_gba, const float* pos_gba,
                                       const int32_t* ref_kf, int n_kf, const uint8_t* reached, const float* Tcw_bef, const float* Twc_new,
                                       float* xw_out, uint8_t* moved) {
  if (const char* e = gba_update_points(n_points, xw, bad, in_gba, pos_gba, ref_kf, n_kf, reached, Tcw_bef, Twc_new, xw_out, moved))
    return obs_invalid("gba_update_points", e);
  return ORBFE_OK;
}

extern "C" int orbfe_correct_loop_mappoints(orbfe_obsgraph* g, orbfe_mappoints* mp, int K, const int32_t* kf_slot, const double* corrected,
                                            const double* noncorrected, const float* Ow_corrected, int n_skip, const int32_t* skip_slot,
                                            const float* scale_factors, int n_levels, int capacity, int32_t* slot_out, int32_t* ref_out,
                                            uint8_t* valid_out, int32_t* count) {
  const char* fn = "correct_loop_mappoints";
  if (!g || !mp || !count || K < 0 || n_skip < 0 || capacity < 0) return obs_invalid(fn, "bad argument");
  if (n_levels < 1 || n_levels > 256) return obs_invalid(fn, "n_levels must be 1 .. 256");
  if (!scale_factors) return obs_invalid(fn, "NULL scale_factors");
  if (capacity > 0 && (!slot_out || !ref_out)) return obs_invalid(fn, "NULL output list");
  if (K > 0 && (!kf_slot || !corrected || !noncorrected || !Ow_corrected)) return obs_invalid(fn, "NULL key-frame array");
  if (n_skip > 0 && !skip_slot) return obs_invalid(fn, "NULL skip list");
  if (const char* e = lc_check_records(K, corrected)) return obs_invalid(fn, e);
  if (const char* e = lc_check_records(K, noncorrected)) return obs_invalid(fn, e);
  if (!lc_finite(Ow_corrected, 3 * (size_t)K)) return obs_invalid(fn, "a camera centre is not finite");
  std::lock_guard<std::mutex> lk(g->m);
  ObsGraphMirror& h = g->h;
  if (const char* e = check_tables(g, mp)) return obs_invalid(fn, e);
  if (const char* e = h.check_kf_list(K, kf_slot)) return obs_invalid(fn, e);  // (also: the rows are enabled)
  if ((int64_t)K * h.kfRowWidth >= ((int64_t)1 << 31)) return obs_invalid(fn, "K * kf_row_width must stay below 2^31");
  if (!h.slots_ok(n_skip, skip_slot)) return obs_invalid(fn, "skip slot outside [0, point_capacity)");
  *count = 0;
  if (K == 0) return ORBFE_OK;
  // the place of every kf slot's first occurrence, and the level check on what the rows can claim
  std::vector<int32_t> firstOf((size_t)K);
  {
    std::unordered_map<int32_t, int32_t> at;
    std::vector<uint8_t> seen((size_t)h.pointCap, 0);
    std::vector<int32_t> cand;
    for (int i = 0; i < n_skip; i++) seen[(size_t)skip_slot[i]] = 1;
    for (int k = 0; k < K; k++) {
      firstOf[(size_t)k] = at.emplace(kf_slot[k], k).first->second;
      if (firstOf[(size_t)k] != k) continue;
      for (int32_t s : h.kfRows[(size_t)kf_slot[k]])
        if (s >= 0 && !seen[(size_t)s]) { seen[(size_t)s] = 1; cand.push_back(s); }
    }
    if (const char* e = h.check_levels((int)cand.size(), cand.data(), n_levels)) return obs_invalid(fn, e);
  }
  MapPointsLock lock(mp);  // the table's own calls have completed and stay out for the scope
  if (lock.rc) return lock.rc;
  if (int rc = obs_kf_ready(g)) return rc;
  const size_t w = (size_t)h.kfRowWidth, nK = (size_t)K, L = (size_t)n_levels, nS = (size_t)n_skip;
  const size_t span = nK * w, nBlocks = (span + kLcBlockEntries - 1) / kLcBlockEntries, nOut = std::min(span, (size_t)h.pointCap);
  Arena* ar = &g->arena;
  LoopCorrectArgs a;
  a.K = K; a.nBlocks = (int)nBlocks; a.nSkip = n_skip; a.nLevels = n_levels;
  int32_t *dKf, *dFirstOf, *dSkip;
  double *dCor, *dNon;
  float *dOw, *dScale;
  auto stage = [&](Arena* s) -> hipError_t {
    TRY(up(s, &dKf, kf_slot, nK));
    TRY(up(s, &dFirstOf, firstOf.data(), nK));
    TRY(up(s, &dCor, corrected, nK * 8));
    TRY(up(s, &dNon, noncorrected, nK * 8));
    TRY(up(s, &dOw, Ow_corrected, nK * 3));
    TRY(up(s, &dScale, scale_factors, L));
    TRY(up(s, &dSkip, skip_slot, nS));
    open_span(s);  // what may come back; how much of it does is decided by the count
    a.count = carve<int32_t>(s, 1);
    a.slotOut = carve<int32_t>(s, nOut);
    a.refOut = carve<int32_t>(s, nOut);
    a.validOut = carve<uint8_t>(s, nOut);
    TRY(close_span(s));
    a.first = carve<int32_t>(s, (size_t)h.pointCap);
    a.keepMask = carve<unsigned long long>(s, nBlocks * kLcChunksPerBlock);
    a.blockCount = carve<int32_t>(s, nBlocks);
    return hipSuccess;
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  RankScope ranks(g);
  if (int rc = ranks.ready()) return rc;
  a.kfSlot = dKf; a.firstOf = dFirstOf; a.skip = dSkip;
  a.corrected = dCor; a.noncorrected = dNon;
  a.owCorrected = dOw; a.scale = dScale;
  a.rank = g->kfRank.p;
  HIPCHK(flush(ar));
  launch_lc_claim(ar->stream, g->d, g->kd, a);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, a.count, a.count + 1));
  HIPCHK(hipStreamSynchronize(ar->stream));  // count first, mutate after
  const int32_t n = *mirror_of(ar, a.count);
  *count = n;
  if (n < 0 || (size_t)n > nOut) return fail(ORBFE_ERR_HIP, std::string(fn) + ": the device returned an impossible count");
  if (n > capacity) {
    launch_lc_release(ar->stream, a);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ar->stream));
    ranks.done = true;
    return fail(ORBFE_ERR_CAPACITY, std::string(fn) + ": more points are claimed than `capacity` (see *count); nothing was changed");
  }
  launch_lc_apply(ar->stream, g->d, g->kd, *lock.table, a, n);
  launch_lc_release(ar->stream, a);
  HIPCHK(hipGetLastError());
  const size_t cnt = (size_t)n;
  if (cnt) {
    HIPCHK(down_range(ar, a.slotOut, a.slotOut + cnt));
    HIPCHK(down_range(ar, a.refOut, a.refOut + cnt));
    if (valid_out) HIPCHK(down_range(ar, a.validOut, a.validOut + cnt));
  }
  HIPCHK(hipStreamSynchronize(ar->stream));
  ranks.done = true;
  if (cnt) {
    std::memcpy(slot_out, mirror_of(ar, a.slotOut), cnt * 4);
    std::memcpy(ref_out, mirror_of(ar, a.refOut), cnt * 4);
    if (valid_out) std::memcpy(valid_out, mirror_of(ar, a.validOut), cnt);
  }
  // the device holds the new centres already: the mirror follows without marking the key frames
  for (int k = 0; k < K; k++) {
    if (firstOf[(size_t)k] != k) continue;
    float* ow = h.kfs[(size_t)kf_slot[k]].ow;
    ow[0] = Ow_corrected[3 * (size_t)k]; ow[1] = Ow_corrected[3 * (size_t)k + 1]; ow[2] = Ow_corrected[3 * (size_t)k + 2];
  }
  return ORBFE_OK;
}

extern "C" int orbfe_gba_update_mappoints(orbfe_obsgraph* g, orbfe_mappoints* mp, int n, const int32_t* slot, const uint8_t* in_gba,
                                          const float* pos_gba, int m, const int32_t* kf_slot, const uint8_t* reached, const float* Tcw_bef,
                                          const float* Twc_new, uint8_t* moved) {
  const char* fn = "gba_update_mappoints";
  if (!g || !mp || n < 0 || m < 0) return obs_invalid(fn, "bad argument");
  if (n > 0 && (!slot || !in_gba || !pos_gba || !moved)) return obs_invalid(fn, "NULL point array");
  if (m > 0 && (!kf_slot || !reached || !Tcw_bef || !Twc_new)) return obs_invalid(fn, "NULL key-frame array");
  for (int i = 0; i < n; i++)
    if (in_gba[i] && !lc_finite(pos_gba + 3 * (size_t)i, 3)) return obs_invalid(fn, "a position is not finite");
  for (int j = 0; j < m; j++)
    if (reached[j] && (!lc_finite(Tcw_bef + 16 * (size_t)j, 16) || !lc_finite(Twc_new + 16 * (size_t)j, 16)))
      return obs_invalid(fn, "a pose is not finite");
  std::lock_guard<std::mutex> lk(g->m);  // what reads the graph's mirror comes behind the lock
  if (const char* e = check_tables(g, mp)) return obs_invalid(fn, e);
  if (n == 0) return ORBFE_OK;
  if (!g->h.slots_ok(n, slot)) return obs_invalid(fn, "slot outside [0, point_capacity)");
  if (!distinct(n, slot)) return obs_invalid(fn, "a slot is named twice");  // it would be rewritten by two lanes
  if (!g->h.kf_slots_ok(m, kf_slot)) return obs_invalid(fn, "kf slot outside [0, kf_capacity)");
  if (!distinct(m, kf_slot)) return obs_invalid(fn, "a kf slot is named twice");
  MapPointsLock lock(mp);
  if (lock.rc) return lock.rc;
  if (int rc = obs_ready(g)) return rc;
  const size_t nP = (size_t)n, nM = (size_t)m;
  Arena* ar = &g->arena;
  GbaUpdateArgs a;
  a.n = n; a.m = m;
  int32_t *dSlot, *dKf;
  uint8_t *dIn, *dReached;
  float *dPos, *dBef, *dNew;
  auto stage = [&](Arena* s) -> hipError_t {
    TRY(up(s, &dSlot, slot, nP));
    TRY(up(s, &dIn, in_gba, nP));
    TRY(up(s, &dPos, pos_gba, nP * 3));
    TRY(up(s, &dKf, kf_slot, nM));
    TRY(up(s, &dReached, reached, nM));
    TRY(up(s, &dBef, Tcw_bef, nM * 16));
    TRY(up(s, &dNew, Twc_new, nM * 16));
    open_span(s);
    a.moved = carve<uint8_t>(s, nP);
    return close_span(s);
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  RankScope ranks(g);
  if (int rc = ranks.ready()) return rc;
  a.slot = dSlot; a.inGba = dIn; a.posGba = dPos;
  a.kfSlot = dKf; a.reached = dReached; a.TcwBef = dBef; a.TwcNew = dNew;
  a.index = g->kfRank.p;
  HIPCHK(flush(ar));
  launch_gba_update(ar->stream, g->d, *lock.table, a);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  ranks.done = true;
  std::memcpy(moved, mirror_of(ar, a.moved), nP);
  return ORBFE_OK;
}
