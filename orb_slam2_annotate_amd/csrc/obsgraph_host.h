// obsgraph_host.h -- the host side of the device observation graph (obsgraph.hip: orbfe_obsgraph_*) that needs no device:
// the mirror of everything the table holds, every argument check, and the two replays that run on one query's votes
// (KeyFrame::UpdateConnections src/KeyFrame.cc:347-393, Tracking::UpdateLocalKeyFrames src/Tracking.cc:1364-1454).
// Plain C++ without a HIP include, so tests/cpp/obsgraph_host_san.cpp runs exactly this code under the address and
// undefined-behaviour sanitizers.
//
// The mirror is the truth: a mutation changes the mirror alone and marks the rows it touched; the next call that reads
// the table on the device rewrites those rows, each as a whole.  Rows are kept in ascending mnId of the observing key
// frame (ties cannot occur: two live kf slots never share an id).
//
// The opposite direction, KeyFrame::mvpMapPoints (key frame -> its points, by keypoint index), lives here too once
// enable_keyframe_points() gave it a width: one row of point slots per kf slot (-1: NULL), under the same discipline.  A
// mirror that never enables it holds nothing more than before.  kfpoints_union_flat() below is the reference's ordered
// union (src/Tracking.cc:1315-1333) over flat arrays: the sanitizer program's check and the CPU yardstick of
// tools/kfpoints_latency.py -- never a fallback, the library does not call it.
//
// The key frames' descriptors (KeyFrame::mDescriptors) are the one thing the handle holds WITHOUT a host copy: they never
// change in the reference, so enable_keyframe_descriptors() gives the store a width and the mirror keeps only descN, the
// number of rows each kf slot received (0: never set).  That is all the checks of the distinctive-descriptor loop need.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <unordered_map>
#include <utility>
#include <vector>

namespace orbfe {

constexpr int kObsMaxPoints = 1 << 24, kObsMaxKeyFrames = 1 << 20;
constexpr int64_t kObsMaxEntries = (int64_t)1 << 28;  // point_capacity * row_width: a 2 GiB table at the most
constexpr int kKfRowMinWidth = 64, kKfRowMaxWidth = 16384;  // kf_row_width: a multiple of 64 (one wave never spans two rows)
constexpr int64_t kKfRowMaxEntries = (int64_t)1 << 28;      // kf_capacity * kf_row_width: a 1 GiB table at the most
constexpr int kKfDescMinWidth = 64, kKfDescMaxWidth = 16384;  // kf_desc_width: a multiple of 64
constexpr int64_t kKfDescMaxRows = (int64_t)1 << 26;          // kf_capacity * kf_desc_width: 2 GiB of 32-byte descriptors at the most

// one observation: 8 bytes, what a lane of the kernels reads
struct ObsEntry {
  int32_t kf;      // kf slot
  uint16_t idx;    // mObservations[pKF]
  uint8_t octave;  // pKF->mvKeysUn[idx].octave
  uint8_t flags;   // bit 0: pKF->mvuRight[idx] >= 0
};
static_assert(sizeof(ObsEntry) == 8, "ObsEntry is 8 bytes");
struct ObsPointMeta { int32_t count, nObs, bad, ref; };  // live entries, MapPoint::nObs, isBad(), mpRefKF's slot (-1: none)
static_assert(sizeof(ObsPointMeta) == 16, "ObsPointMeta is 16 bytes");
struct ObsKeyFrame {
  int64_t id;  // mnId; -1: the slot was never set
  float ow[3];
  int32_t bad;
};
static_assert(sizeof(ObsKeyFrame) == 24, "ObsKeyFrame is 24 bytes");

inline const char* obsgraph_check_create(int device, int point_capacity, int kf_capacity, int row_width, const void* out) {
  if (!out) return "NULL argument";
  if (device < 0) return "negative device";
  if (point_capacity <= 0 || point_capacity > kObsMaxPoints) return "point_capacity must be 1 .. 16777216";
  if (kf_capacity <= 0 || kf_capacity > kObsMaxKeyFrames) return "kf_capacity must be 1 .. 1048576";
  if (row_width < 8 || row_width > 256 || (row_width & (row_width - 1))) return "row_width must be a power of two in 8 .. 256";
  if ((int64_t)point_capacity * row_width > kObsMaxEntries) return "point_capacity * row_width must not exceed 2^28";
  return nullptr;
}

struct ObsGraphMirror {
  int pointCap = 0, kfCap = 0, rowWidth = 0;
  std::vector<std::vector<ObsEntry>> rows;
  std::vector<ObsPointMeta> meta;
  std::vector<ObsKeyFrame> kfs;
  std::vector<int32_t> kfRefs;                   // entries that name the kf slot
  std::vector<std::vector<int32_t>> kfPoints;    // point slots that named the kf slot since it was set (may be stale)
  std::unordered_map<int64_t, int32_t> slotOfId;  // mnId -> kf slot
  // what the device has not seen yet
  std::vector<uint8_t> rowDirty;
  std::vector<int32_t> dirtyRows;
  int kfDirtyLo = 0, kfDirtyHi = 0;  // [lo, hi)
  // KeyFrame::mvpMapPoints per kf slot; kfRowWidth = 0: not enabled, and nothing below is allocated
  int kfRowWidth = 0;
  std::vector<std::vector<int32_t>> kfRows;
  std::vector<uint8_t> kfRowDirty;
  std::vector<int32_t> dirtyKfRows;
  // KeyFrame::mDescriptors per kf slot: the bytes are on the device alone; kfDescWidth = 0: not enabled
  int kfDescWidth = 0;
  std::vector<int32_t> descN;  // rows the kf slot received (0: never set)

  void init(int points, int keyframes, int width) {
    pointCap = points; kfCap = keyframes; rowWidth = width;
    rows.assign((size_t)points, {});
    meta.assign((size_t)points, ObsPointMeta{0, 0, 1, -1});  // a slot that was never set counts as bad
    kfs.assign((size_t)keyframes, ObsKeyFrame{-1, {0.f, 0.f, 0.f}, 1});
    kfRefs.assign((size_t)keyframes, 0);
    kfPoints.assign((size_t)keyframes, {});
    slotOfId.clear();
    rowDirty.assign((size_t)points, 0);
    dirtyRows.clear();
    kfDirtyLo = 0; kfDirtyHi = keyframes;
  }
  // what clear() leaves: as after create; everything is marked for the device
  void clear() {
    init(pointCap, kfCap, rowWidth);
    for (int s = 0; s < pointCap; s++) touch(s);
    if (kfRowWidth) {  // the rows are emptied, the width stays
      kfRows.assign((size_t)kfCap, {});
      for (int k = 0; k < kfCap; k++) touch_kf_row(k);
    }
    if (kfDescWidth) descN.assign((size_t)kfCap, 0);  // the width and the device slab stay
  }
  void touch(int slot) {
    if (!rowDirty[(size_t)slot]) { rowDirty[(size_t)slot] = 1; dirtyRows.push_back(slot); }
  }
  void touch_kf(int k) {
    if (kfDirtyLo >= kfDirtyHi) { kfDirtyLo = k; kfDirtyHi = k + 1; }
    else { kfDirtyLo = std::min(kfDirtyLo, k); kfDirtyHi = std::max(kfDirtyHi, k + 1); }
  }
  void flushed() {
    for (int32_t s : dirtyRows) rowDirty[(size_t)s] = 0;
    dirtyRows.clear();
    kfDirtyLo = kfDirtyHi = 0;
  }
  // every row, the whole key-frame range: what a table that was just allocated needs
  void mark_all() {
    for (int s = 0; s < pointCap; s++) touch(s);
    kfDirtyLo = 0; kfDirtyHi = kfCap;
  }

  bool slots_ok(int n, const int32_t* slot) const {
    for (int i = 0; i < n; i++)
      if (slot[i] < 0 || slot[i] >= pointCap) return false;
    return true;
  }
  bool kf_slots_ok(int n, const int32_t* kf) const {
    for (int i = 0; i < n; i++)
      if (kf[i] < 0 || kf[i] >= kfCap) return false;
    return true;
  }
  int find(int slot, int kf) const {
    const std::vector<ObsEntry>& r = rows[(size_t)slot];
    for (size_t i = 0; i < r.size(); i++)
      if (r[i].kf == kf) return (int)i;
    return -1;
  }

  // NULL when done, else what is wrong (nothing applied)
  const char* set_keyframes(int n, const int32_t* kf, const int64_t* id, const float* ow, const uint8_t* bad) {
    if (n < 0) return "negative count";
    if (n == 0) return nullptr;
    if (!kf || !id || !ow || !bad) return "NULL array";
    if (!kf_slots_ok(n, kf)) return "kf slot outside [0, kf_capacity)";
    // checked on a copy of the id map: the call applies as a whole or not at all
    std::unordered_map<int64_t, int32_t> ids = slotOfId;
    std::vector<int64_t> cur((size_t)n);
    for (int i = 0; i < n; i++) {
      if (id[i] < 0) return "negative key-frame id";
      const int64_t old = kfs[(size_t)kf[i]].id;
      int64_t held = old;
      for (int j = 0; j < i; j++)
        if (kf[j] == kf[i]) held = id[j];  // the slot's id after the earlier entries of this call
      if (held != id[i]) {
        if (kfRefs[(size_t)kf[i]] > 0) return "the id of a key frame that rows name cannot change";
        auto it = ids.find(id[i]);
        if (it != ids.end() && it->second != kf[i]) return "key-frame id already held by another kf slot";
        if (held >= 0) ids.erase(held);
        ids[id[i]] = kf[i];
      }
    }
    for (int i = 0; i < n; i++) {
      ObsKeyFrame& k = kfs[(size_t)kf[i]];
      if (k.id != id[i]) kfPoints[(size_t)kf[i]].clear();
      k.id = id[i];
      k.ow[0] = ow[3 * i]; k.ow[1] = ow[3 * i + 1]; k.ow[2] = ow[3 * i + 2];
      k.bad = bad[i] ? 1 : 0;
      touch_kf(kf[i]);
    }
    slotOfId.swap(ids);
    return nullptr;
  }

  const char* set_points(int n, const int32_t* slot, const uint8_t* bad, const int32_t* ref) {
    if (n < 0) return "negative count";
    if (n == 0) return nullptr;
    if (!slot || !bad || !ref) return "NULL array";
    if (!slots_ok(n, slot)) return "slot outside [0, point_capacity)";
    for (int i = 0; i < n; i++)
      if (ref[i] < -1 || ref[i] >= kfCap) return "ref_kf_slot outside [-1, kf_capacity)";
    for (int i = 0; i < n; i++) {
      ObsPointMeta& m = meta[(size_t)slot[i]];
      m.bad = bad[i] ? 1 : 0;
      m.ref = ref[i];
      if (m.count == 0) m.nObs = 0;  // an empty row starts again
      touch(slot[i]);
    }
    return nullptr;
  }

  // MapPoint::AddObservation (src/MapPoint.cc:101-114).  *full: a row has no room (nothing of the call applied)
  const char* add_observations(int n, const int32_t* slot, const int32_t* kf, const uint16_t* idx, const uint8_t* octave,
                               const uint8_t* stereo, bool* full) {
    *full = false;
    if (n < 0) return "negative count";
    if (n == 0) return nullptr;
    if (!slot || !kf || !idx || !octave || !stereo) return "NULL array";
    if (!slots_ok(n, slot)) return "slot outside [0, point_capacity)";
    if (!kf_slots_ok(n, kf)) return "kf slot outside [0, kf_capacity)";
    for (int i = 0; i < n; i++)
      if (kfs[(size_t)kf[i]].id < 0) return "kf slot was never set (orbfe_obsgraph_set_keyframes)";
    std::unordered_map<int32_t, std::pair<std::vector<ObsEntry>, ObsPointMeta>> undo;
    std::vector<std::pair<int32_t, int32_t>> added;  // (kf, slot)
    for (int i = 0; i < n; i++) {
      const int s = slot[i];
      if (find(s, kf[i]) >= 0) continue;  // mObservations.count(pKF): return
      std::vector<ObsEntry>& r = rows[(size_t)s];
      if ((int)r.size() >= rowWidth) {
        for (auto& u : undo) { rows[(size_t)u.first] = u.second.first; meta[(size_t)u.first] = u.second.second; }
        for (auto& a : added) { kfRefs[(size_t)a.first]--; kfPoints[(size_t)a.first].pop_back(); }
        *full = true;
        return "a row is full (row_width observations)";
      }
      if (!undo.count(s)) undo.emplace(s, std::make_pair(r, meta[(size_t)s]));
      const ObsEntry e = {kf[i], idx[i], octave[i], (uint8_t)(stereo[i] ? 1 : 0)};
      const int64_t id = kfs[(size_t)kf[i]].id;
      size_t at = 0;
      while (at < r.size() && kfs[(size_t)r[at].kf].id < id) at++;
      r.insert(r.begin() + (ptrdiff_t)at, e);
      ObsPointMeta& m = meta[(size_t)s];
      m.count = (int32_t)r.size();
      m.nObs += stereo[i] ? 2 : 1;
      kfRefs[(size_t)kf[i]]++;
      kfPoints[(size_t)kf[i]].push_back(s);
      added.emplace_back(kf[i], s);
    }
    for (auto& u : undo) touch(u.first);
    return nullptr;
  }

  // MapPoint::EraseObservation (:119-145) with the part of SetBadFlag (:164-182) that concerns the table; true when the
  // point became bad
  bool erase_one(int s, int k) {
    const int at = find(s, k);
    if (at < 0) return false;
    std::vector<ObsEntry>& r = rows[(size_t)s];
    ObsPointMeta& m = meta[(size_t)s];
    m.nObs -= (r[(size_t)at].flags & 1) ? 2 : 1;
    r.erase(r.begin() + at);
    kfRefs[(size_t)k]--;
    if (m.ref == k) m.ref = r.empty() ? -1 : r[0].kf;  // mObservations.begin()->first, in this table's order
    bool bad = false;
    if (m.nObs <= 2) {
      bad = true;
      m.bad = 1;
      for (const ObsEntry& e : r) kfRefs[(size_t)e.kf]--;
      r.clear();
    }
    m.count = (int32_t)r.size();
    touch(s);
    return bad;
  }

  const char* erase_observations(int n, const int32_t* slot, const int32_t* kf, uint8_t* became_bad) {
    if (n < 0) return "negative count";
    if (n == 0) return nullptr;
    if (!slot || !kf) return "NULL array";
    if (!slots_ok(n, slot)) return "slot outside [0, point_capacity)";
    if (!kf_slots_ok(n, kf)) return "kf slot outside [0, kf_capacity)";
    for (int i = 0; i < n; i++) {
      const bool b = erase_one(slot[i], kf[i]);
      if (became_bad) became_bad[i] = b ? 1 : 0;
    }
    return nullptr;
  }

  // the map-point part of KeyFrame::SetBadFlag (src/KeyFrame.cc:488 ff.).  *over: more points become bad than `capacity`
  // (*n_out set, nothing applied)
  const char* erase_keyframe(int k, int32_t* out, int capacity, int* n_out, bool* over) {
    *over = false;
    if (!n_out || capacity < 0 || (capacity > 0 && !out)) return "bad argument";
    *n_out = 0;
    if (k < 0 || k >= kfCap) return "kf slot outside [0, kf_capacity)";
    std::vector<int32_t> pts = kfPoints[(size_t)k];
    std::sort(pts.begin(), pts.end());
    pts.erase(std::unique(pts.begin(), pts.end()), pts.end());
    int nBad = 0;
    for (int32_t s : pts) {
      const int at = find(s, k);
      if (at >= 0 && meta[(size_t)s].nObs - ((rows[(size_t)s][(size_t)at].flags & 1) ? 2 : 1) <= 2) nBad++;
    }
    *n_out = nBad;
    if (nBad > capacity) { *over = true; return "more points became bad than `capacity` (see n_out)"; }
    int w = 0;
    for (int32_t s : pts)
      if (erase_one(s, k)) out[w++] = s;
    kfPoints[(size_t)k].clear();
    kfs[(size_t)k].bad = 1;
    touch_kf(k);
    return nullptr;
  }

  // what update_normal_depth needs to know before it may launch: a reference entry whose octave is no pyramid level
  const char* check_levels(int n, const int32_t* slot, int n_levels) const {
    for (int i = 0; i < n; i++) {
      const ObsPointMeta& m = meta[(size_t)slot[i]];
      if (m.bad || m.count == 0 || m.ref < 0) continue;
      const int at = find(slot[i], m.ref);
      if (at >= 0 && rows[(size_t)slot[i]][(size_t)at].octave >= n_levels) return "a reference observation's octave is not below n_levels";
    }
    return nullptr;
  }

  // Everything set_points(bad = 0, ref = kf), add_observations(slot, kf, idx < nIdx, ..) and -- rows enabled --
  // assign_keyframe_points(kf, idx < nIdx, slot) of n NEW points can refuse, for a caller that must know before it touches
  // the device (stereopoints.hip): NULL when the three mutators will accept the points.  Distinct slots are the caller's.
  const char* check_new_points(int n, const int32_t* slot, int kf, int nIdx) const {
    if (kf < 0 || kf >= kfCap || kfs[(size_t)kf].id < 0) return "kf_slot was never set (orbfe_obsgraph_set_keyframes)";
    if (rowWidth < 1) return "the rows hold no observation";
    for (int j = 0; j < n; j++) {
      if (slot[j] < 0 || slot[j] >= pointCap) return "a new slot is at or past the graph's point capacity";
      const ObsPointMeta& m = meta[(size_t)slot[j]];
      if (!m.bad || m.count != 0 || !rows[(size_t)slot[j]].empty()) return "a new slot's graph row is live";
    }
    if (nIdx > 65536) return "a keypoint index does not fit an observation";
    if (kfRowWidth && (int)kfRows[(size_t)kf].size() < nIdx) return "kf_slot's row of map points is shorter than n";
    return nullptr;
  }

  // The same question for n NEW points with TWO observations each, by key frame kf[0] and by one of kf[1 .. nKf) (tripoints.hip):
  // set_points(bad = 0, ref = kf[0]), two add_observations per point with idx < nIdx[j] for key frame kf[j], and -- rows
  // enabled -- assign_keyframe_points for both.  Also refused, because ComputeDistinctiveDescriptors and UpdateNormalAndDepth
  // for the row of two would not be what the caller computes: a bad key frame, a kf slot named twice, two equal mnIds.
  // Distinct point slots are the caller's.
  const char* check_new_pair_points(int n, const int32_t* slot, int nKf, const int32_t* kf, const int32_t* nIdx) const {
    if (rowWidth < 2) return "the rows do not hold two observations";
    for (int j = 0; j < nKf; j++) {
      if (kf[j] < 0 || kf[j] >= kfCap || kfs[(size_t)kf[j]].id < 0) return "a kf slot is out of range or was never set (orbfe_obsgraph_set_keyframes)";
      if (kfs[(size_t)kf[j]].bad) return "a key frame is bad";
      for (int i = 0; i < j; i++)
        if (kf[i] == kf[j] || kfs[(size_t)kf[i]].id == kfs[(size_t)kf[j]].id) return "a key frame is named twice";
      if (nIdx[j] > 65536) return "a keypoint index does not fit an observation";
      if (kfRowWidth && (int)kfRows[(size_t)kf[j]].size() < nIdx[j]) return "a key frame's row of map points is shorter than its frame";
    }
    for (int j = 0; j < n; j++) {
      if (slot[j] < 0 || slot[j] >= pointCap) return "a new slot is at or past the graph's point capacity";
      const ObsPointMeta& m = meta[(size_t)slot[j]];
      if (!m.bad || m.count != 0 || !rows[(size_t)slot[j]].empty()) return "a new slot's graph row is live";
    }
    return nullptr;
  }

  // ---- KeyFrame::mvpMapPoints (src/KeyFrame.cc:220-243) ----

  void touch_kf_row(int k) {
    if (!kfRowDirty[(size_t)k]) { kfRowDirty[(size_t)k] = 1; dirtyKfRows.push_back(k); }
  }
  void kf_rows_flushed() {
    for (int32_t k : dirtyKfRows) kfRowDirty[(size_t)k] = 0;
    dirtyKfRows.clear();
  }
  // what a slab of rows that was just allocated needs: the rows that hold something (the lengths travel as one block)
  void mark_kf_rows_held() {
    kf_rows_flushed();
    for (int k = 0; k < kfCap; k++)
      if (!kfRows[(size_t)k].empty()) touch_kf_row(k);
  }

  const char* enable_keyframe_points(int width) {
    if (width < kKfRowMinWidth || width > kKfRowMaxWidth || width % 64) return "kf_row_width must be a multiple of 64 in 64 .. 16384";
    if ((int64_t)kfCap * width > kKfRowMaxEntries) return "kf_capacity * kf_row_width must not exceed 2^28";
    if (kfRowWidth) return kfRowWidth == width ? nullptr : "key-frame rows are enabled with another width";
    kfRows.assign((size_t)kfCap, {});
    kfRowDirty.assign((size_t)kfCap, 0);
    dirtyKfRows.clear();
    kfRowWidth = width;
    return nullptr;
  }

  // the whole mvpMapPoints of a key frame, as at the KeyFrame constructor (N = n entries, -1: NULL)
  const char* set_keyframe_points(int k, int n, const int32_t* slot) {
    if (!kfRowWidth) return "key-frame rows are not enabled (orbfe_obsgraph_enable_keyframe_points)";
    if (k < 0 || k >= kfCap) return "kf slot outside [0, kf_capacity)";
    if (kfs[(size_t)k].id < 0) return "kf slot was never set (orbfe_obsgraph_set_keyframes)";
    if (n < 0 || n > kfRowWidth) return "n outside [0, kf_row_width]";
    if (n > 0 && !slot) return "NULL array";
    for (int i = 0; i < n; i++)
      if (slot[i] < -1 || slot[i] >= pointCap) return "slot outside [-1, point_capacity)";
    kfRows[(size_t)k].assign(slot, slot + n);
    touch_kf_row(k);
    return nullptr;
  }

  // AddMapPoint / ReplaceMapPointMatch (mvpMapPoints[idx] = pMP) and EraseMapPointMatch(idx) (slot -1), n times in order;
  // everything is checked before the first entry changes
  const char* assign_keyframe_points(int n, const int32_t* kf, const uint16_t* idx, const int32_t* slot) {
    if (!kfRowWidth) return "key-frame rows are not enabled (orbfe_obsgraph_enable_keyframe_points)";
    if (n < 0) return "negative count";
    if (n == 0) return nullptr;
    if (!kf || !idx || !slot) return "NULL array";
    if (!kf_slots_ok(n, kf)) return "kf slot outside [0, kf_capacity)";
    for (int i = 0; i < n; i++) {
      if ((size_t)idx[i] >= kfRows[(size_t)kf[i]].size()) return "idx is not below the row's length";
      if (slot[i] < -1 || slot[i] >= pointCap) return "slot outside [-1, point_capacity)";
    }
    for (int i = 0; i < n; i++) {
      kfRows[(size_t)kf[i]][idx[i]] = slot[i];
      touch_kf_row(kf[i]);
    }
    return nullptr;
  }

  // the key-frame lists of n_queries union queries (offsets as in orbfe_obsgraph_votes): NULL when they may be enqueued
  const char* check_kf_queries(int nQueries, const int32_t* off, const int32_t* kf) const {
    if (!kfRowWidth) return "key-frame rows are not enabled (orbfe_obsgraph_enable_keyframe_points)";
    if (off[0] != 0) return "q_offsets[0] must be 0";
    for (int q = 0; q < nQueries; q++) {
      if (off[q + 1] < off[q]) return "q_offsets must not descend";
      if ((int64_t)(off[q + 1] - off[q]) * kfRowWidth >= ((int64_t)1 << 31)) return "a query's key frames * kf_row_width must stay below 2^31";
    }
    if (off[nQueries] > 0 && !kf) return "NULL q_kf_slots";
    return check_kf_list(off[nQueries], kf);
  }
  const char* check_kf_list(int n, const int32_t* kf) const {
    if (!kfRowWidth) return "key-frame rows are not enabled (orbfe_obsgraph_enable_keyframe_points)";
    if (!kf_slots_ok(n, kf)) return "kf slot outside [0, kf_capacity)";
    for (int i = 0; i < n; i++)
      if (kfs[(size_t)kf[i]].id < 0) return "kf slot was never set (orbfe_obsgraph_set_keyframes)";
    return nullptr;
  }

  // ---- KeyFrame::mDescriptors and MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) ----

  const char* enable_keyframe_descriptors(int width) {
    if (width < kKfDescMinWidth || width > kKfDescMaxWidth || width % 64) return "kf_desc_width must be a multiple of 64 in 64 .. 16384";
    if ((int64_t)kfCap * width > kKfDescMaxRows) return "kf_capacity * kf_desc_width must not exceed 2^26";
    if (kfDescWidth) return kfDescWidth == width ? nullptr : "key-frame descriptors are enabled with another width";
    descN.assign((size_t)kfCap, 0);
    kfDescWidth = width;
    return nullptr;
  }

  // what either set_keyframe_descriptors call checks before it touches the device (have: the source is there)
  const char* check_set_keyframe_descriptors(int k, int n, bool have) const {
    if (!kfDescWidth) return "key-frame descriptors are not enabled (orbfe_obsgraph_enable_keyframe_descriptors)";
    if (k < 0 || k >= kfCap) return "kf slot outside [0, kf_capacity)";
    if (kfs[(size_t)k].id < 0) return "kf slot was never set (orbfe_obsgraph_set_keyframes)";
    if (n < 0 || n > kfDescWidth) return "n outside [0, kf_desc_width]";
    if (n > 0 && !have) return "NULL descriptors";
    return nullptr;
  }

  // what the distinctive-descriptor loop needs to know before it may launch: every entry the kernel can gather -- the
  // entries of a listed point that is not bad, whether or not the entry's key frame is bad -- names a descriptor row
  // that was set.  A bad point's row is never read on the device, so it is not looked at here either.
  const char* check_distinctive(int n, const int32_t* slot) const {
    if (!kfDescWidth) return "key-frame descriptors are not enabled (orbfe_obsgraph_enable_keyframe_descriptors)";
    if (!slots_ok(n, slot)) return "slot outside [0, point_capacity)";
    for (int i = 0; i < n; i++) {
      if (meta[(size_t)slot[i]].bad) continue;
      for (const ObsEntry& e : rows[(size_t)slot[i]]) {
        const int32_t have = descN[(size_t)e.kf];
        if (have == 0) return "an observing key frame's descriptors were never set (orbfe_obsgraph_set_keyframe_descriptors)";
        if ((int32_t)e.idx >= have) return "an observation's idx is not below its key frame's descriptor count";
      }
    }
    return nullptr;
  }
};

// ---- host replays over one query's votes ----

// ascending-id order of n (id, ...) records; false when an id repeats
inline bool obs_order_by_id(int n, const int64_t* id, std::vector<int>* order) {
  order->resize((size_t)n);
  for (int i = 0; i < n; i++) (*order)[(size_t)i] = i;
  std::sort(order->begin(), order->end(), [&](int a, int b) { return id[a] < id[b]; });
  for (int i = 1; i < n; i++)
    if (id[(*order)[(size_t)i]] == id[(*order)[(size_t)i - 1]]) return false;
  return true;
}

// KeyFrame::UpdateConnections :347-393 on KFcounter = (kf_id, weight)[n].  ordered_*: mvpOrderedConnectedKeyFrames /
// mvOrderedWeights; connect_*: who receives AddConnection(this, weight), in KFcounter's (ascending id) order; parent:
// mvpOrderedConnectedKeyFrames.front().  Every output array holds n entries.  NULL when done.
inline const char* obsgraph_update_connections(int n, const int64_t* kf_id, const int32_t* weight, int th, int64_t* ordered_id,
                                               int32_t* ordered_weight, int* n_ordered, int64_t* connect_id,
                                               int32_t* connect_weight, int* n_connect, int64_t* parent_id) {
  if (n < 0 || !n_ordered || !n_connect || !parent_id) return "bad argument";
  *n_ordered = *n_connect = 0;
  *parent_id = -1;
  if (n == 0) return nullptr;  // KFcounter.empty(): return (:347)
  if (!kf_id || !weight || !ordered_id || !ordered_weight || !connect_id || !connect_weight) return "NULL array";
  for (int i = 0; i < n; i++)
    if (weight[i] <= 0) return "a counter entry must be positive";
  std::vector<int> order;
  if (!obs_order_by_id(n, kf_id, &order)) return "a key-frame id is named twice";
  int nmax = 0;
  int64_t kfmax = -1;
  std::vector<std::pair<int32_t, int64_t>> pairs;
  int nc = 0;
  for (int i : order) {
    if (weight[i] > nmax) { nmax = weight[i]; kfmax = kf_id[i]; }
    if (weight[i] >= th) {
      pairs.emplace_back(weight[i], kf_id[i]);
      connect_id[nc] = kf_id[i]; connect_weight[nc] = weight[i]; nc++;
    }
  }
  if (pairs.empty()) {
    pairs.emplace_back(nmax, kfmax);
    connect_id[0] = kfmax; connect_weight[0] = nmax; nc = 1;
  }
  std::sort(pairs.begin(), pairs.end());  // pair<int, KeyFrame*>: by weight, then by key frame (here: by id)
  const int m = (int)pairs.size();
  for (int i = 0; i < m; i++) {  // push_front
    ordered_id[m - 1 - i] = pairs[(size_t)i].second;
    ordered_weight[m - 1 - i] = pairs[(size_t)i].first;
  }
  *n_ordered = m;
  *n_connect = nc;
  *parent_id = ordered_id[0];
  return nullptr;
}

// Tracking::UpdateLocalKeyFrames :1364-1454 on keyframeCounter = (kf_id, weight, bad)[n].  Record i also carries what
// the K2 walk reads of key frame i: GetBestCovisibilityKeyFrames (the whole ordered list may be given; the first 10 are
// read) as neigh_id / neigh_bad [neigh_off[i], neigh_off[i+1]), GetChilds() likewise (ascending id), GetParent() as
// parent_id[i] (-1: none).  out_id: mvpLocalKeyFrames, *n_out of them; *ref_id: pKFmax (-1: none).  *over: more than
// `capacity` (*n_out set).  NULL when done.
inline const char* obsgraph_local_keyframes(int n, const int64_t* kf_id, const int32_t* weight, const uint8_t* bad,
                                            const int32_t* neigh_off, const int64_t* neigh_id, const uint8_t* neigh_bad,
                                            const int32_t* child_off, const int64_t* child_id, const uint8_t* child_bad,
                                            const int64_t* parent_id, int64_t* out_id, int capacity, int* n_out, int64_t* ref_id,
                                            bool* over) {
  *over = false;
  if (n < 0 || capacity < 0 || !n_out || !ref_id || (capacity > 0 && !out_id)) return "bad argument";
  *n_out = 0;
  *ref_id = -1;
  if (n == 0) return nullptr;  // keyframeCounter.empty(): return (:1364)
  if (!kf_id || !weight || !bad || !neigh_off || !child_off || !parent_id) return "NULL array";
  if (neigh_off[0] != 0 || child_off[0] != 0) return "offsets must start at 0";
  for (int i = 0; i < n; i++)
    if (neigh_off[i + 1] < neigh_off[i] || child_off[i + 1] < child_off[i]) return "offsets must not descend";
  if ((neigh_off[n] > 0 && (!neigh_id || !neigh_bad)) || (child_off[n] > 0 && (!child_id || !child_bad))) return "NULL array";
  std::vector<int> order;
  if (!obs_order_by_id(n, kf_id, &order)) return "a key-frame id is named twice";
  std::vector<int64_t> local;
  std::vector<int> rec;  // record of local[i], for the K1 part
  std::unordered_map<int64_t, char> tracked;  // mnTrackReferenceForFrame == mCurrentFrame.mnId
  int max = 0;
  for (int i : order) {  // K1 (:1374-1389)
    if (bad[i]) continue;
    if (weight[i] > max) { max = weight[i]; *ref_id = kf_id[i]; }
    local.push_back(kf_id[i]);
    rec.push_back(i);
    tracked[kf_id[i]] = 1;
  }
  // K2 (:1393-1448): the loop's end iterator is taken before anything is appended, so it visits K1 alone -- the vector
  // grows under it (reserve(3 * size) keeps the iterators valid) and the size() > 80 stop reads the grown size
  const size_t k1 = local.size();
  for (size_t it = 0; it < k1; it++) {
    if (local.size() > 80) break;
    const int i = rec[it];
    const int nb = std::min(neigh_off[i + 1], neigh_off[i] + 10);  // GetBestCovisibilityKeyFrames(10)
    for (int j = neigh_off[i]; j < nb; j++) {
      if (neigh_bad[j] || tracked.count(neigh_id[j])) continue;
      local.push_back(neigh_id[j]);
      tracked[neigh_id[j]] = 1;
      break;
    }
    for (int j = child_off[i]; j < child_off[i + 1]; j++) {
      if (child_bad[j] || tracked.count(child_id[j])) continue;
      local.push_back(child_id[j]);
      tracked[child_id[j]] = 1;
      break;
    }
    if (parent_id[i] >= 0 && !tracked.count(parent_id[i])) {
      local.push_back(parent_id[i]);
      tracked[parent_id[i]] = 1;
      break;  // (:1444) leaves the whole loop
    }
  }
  *n_out = (int)local.size();
  const size_t m = std::min(local.size(), (size_t)capacity);
  for (size_t i = 0; i < m; i++) out_id[i] = local[i];
  if (local.size() > (size_t)capacity) { *over = true; return "more local key frames than `capacity` (see n_out)"; }
  return nullptr;
}

// ---- the loops over mvpMapPoints on flat arrays: rows [kf][width] of point slots, len [kf], meta [point] ----

// The ordered union of Tracking::UpdateLocalPoints (src/Tracking.cc:1315-1333; the same loop as
// LocalMapping::SearchInNeighbors src/LocalMapping.cc:555-571, LoopClosing::ComputeSim3 src/LoopClosing.cc:420-436 and
// lLocalMapPoints of Optimizer::LocalBundleAdjustment): key frames in list order, entries in idx order, NULL (-1) skipped,
// a point stamped for this query skipped (mnTrackReferenceForFrame == mCurrentFrame.mnId), bad points skipped, the rest
// emitted and stamped.  stamp: one int32 per point slot, every entry different from `mark` on entry (the caller raises
// mark from query to query, as the reference raises the frame id).  Returns the count; out receives the first `capacity`.
inline int kfpoints_union_flat(const int32_t* rows, const int32_t* len, int width, const ObsPointMeta* meta, int nKf,
                               const int32_t* kf, int32_t* stamp, int32_t mark, int32_t* out, int capacity) {
  int n = 0;
  for (int k = 0; k < nKf; k++) {
    const int32_t* r = rows + (size_t)kf[k] * (size_t)width;
    const int m = len[kf[k]];
    for (int i = 0; i < m; i++) {
      const int32_t s = r[i];
      if (s < 0) continue;               // !pMP
      if (stamp[s] == mark) continue;    // already a local point of this query
      if (meta[s].bad) continue;         // isBad() (a slot that was never set counts as bad)
      if (n < capacity) out[n] = s;
      n++;
      stamp[s] = mark;
    }
  }
  return n;
}

// MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:288-328) of one row on flat arrays: entries [count] in the
// table's order, kfBad [kf], desc [kf][width][32].  Returns the row position of the winner, -1 when no entry remains.  The
// sanitizer program's check and a CPU yardstick -- never a fallback, the library does not call it.
inline int obsdesc_distinctive_flat(const ObsEntry* entries, int count, const ObsKeyFrame* kf, const uint8_t* desc, int width) {
  std::vector<int> live;
  for (int e = 0; e < count; e++)
    if (!kf[entries[e].kf].bad) live.push_back(e);  // !pKF->isBad() (:292)
  const int N = (int)live.size();
  if (N == 0) return -1;  // vDescriptors.empty(): return (:296)
  auto row = [&](int e) { return desc + ((size_t)entries[e].kf * (size_t)width + entries[e].idx) * 32; };
  int bestMedian = 1 << 30, best = -1;
  std::vector<int> d((size_t)N);
  for (int i = 0; i < N; i++) {
    for (int j = 0; j < N; j++) {
      int s = 0;
      for (int b = 0; b < 32; b++) s += __builtin_popcount((unsigned)(row(live[(size_t)i])[b] ^ row(live[(size_t)j])[b]));
      d[(size_t)j] = s;
    }
    std::sort(d.begin(), d.end());
    const int median = d[(size_t)(0.5 * (N - 1))];  // (:321)
    if (median < bestMedian) { bestMedian = median; best = live[(size_t)i]; }  // strict <: the first row wins (:323)
  }
  return best;
}

// KeyFrame::TrackedMapPoints (src/KeyFrame.cc:264-289) of one row
inline int kfpoints_tracked_flat(const int32_t* row, int len, const ObsPointMeta* meta, int minObs) {
  int n = 0;
  for (int i = 0; i < len; i++) {
    const int32_t s = row[i];
    if (s < 0 || meta[s].bad) continue;
    if (minObs > 0 ? meta[s].nObs >= minObs : true) n++;
  }
  return n;
}

}  // namespace orbfe
