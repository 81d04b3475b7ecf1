// kfpoints.hip -- host side of the key-frame rows of the device observation graph (include/orbfe.h:
// orbfe_obsgraph_*keyframe_points*, orbfe_obsgraph_tracked_points; kernels: k_kfpoints.hip).  Reference:
// KeyFrame::mvpMapPoints and the loops over it -- Tracking::UpdateLocalPoints (src/Tracking.cc:1311-1334),
// LocalMapping::SearchInNeighbors (src/LocalMapping.cc:552-571), LoopClosing::ComputeSim3 (src/LoopClosing.cc:417-436),
// KeyFrame::TrackedMapPoints (src/KeyFrame.cc:264-289).
//
// The rows live in a slab of their own: int32 rows [kf_capacity][kf_row_width] and one length per kf slot, taken at the
// first device call after enable.  The discipline is obsgraph.hip's: the mirror (obsgraph_host.h) is the truth, mutations
// mark rows, a reading call rewrites the marked rows whole, every operand is checked before anything is enqueued, and
// everything runs on the handle's one stream and is complete on return.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "host_internal.h"
#include "obsgraph_handle.h"
#include "obsgraph_host.h"
#include "obsgraph_kernels.h"

using namespace orbfe;

namespace {

// what one group of union queries may take: first[] entries, blocks of the flat grid (2^21 * 1024 positions < 2^32
// threads / 4 entries each), staged output entries
constexpr size_t kUnionMaxFirst = (size_t)1 << 26, kUnionMaxBlocks = (size_t)1 << 21, kUnionMaxOut = (size_t)1 << 26;
// up to this many bytes the counts and the lists come back in one copy; above, the counts first and then the filled part
constexpr size_t kUnionOneCopyBytes = (size_t)256 << 10;

// the marked key-frame rows onto the device; the marks are dropped only when everything has arrived
int kf_flush(orbfe_obsgraph* g) {
  ObsGraphMirror& h = g->h;
  Arena* ar = &g->arena;
  const size_t w = (size_t)h.kfRowWidth;
  const size_t perRow = 12 + w * 4;
  const size_t rowsPerChunk = std::max<size_t>(1, kObsFlushChunkBytes / perRow);
  for (size_t at = 0; at < h.dirtyKfRows.size(); at += rowsPerChunk) {
    const size_t n = std::min(rowsPerChunk, h.dirtyKfRows.size() - at);
    const int32_t* marked = h.dirtyKfRows.data() + at;
    size_t nRows = 0;
    for (size_t i = 0; i < n; i++) nRows += !h.kfRows[(size_t)marked[i]].empty();
    int32_t *dKf, *dLen, *dRowOf, *dRows;
    auto stage = [&](Arena* a) -> hipError_t {
      TRY(up(a, &dKf, marked, n));
      TRY(up_pack(a, &dLen, n, [&](int32_t* len) {
        for (size_t i = 0; i < n; i++) len[i] = (int32_t)h.kfRows[(size_t)marked[i]].size();
      }));
      TRY(up_pack(a, &dRowOf, n, [&](int32_t* rowOf) {
        int32_t r = 0;
        for (size_t i = 0; i < n; i++) rowOf[i] = h.kfRows[(size_t)marked[i]].empty() ? -1 : r++;
      }));
      return up_pack(a, &dRows, nRows * w, [&](int32_t* rows) {  // the rows that hold something, each padded with -1
        for (size_t i = 0; i < n; i++) {
          const std::vector<int32_t>& row = h.kfRows[(size_t)marked[i]];
          if (row.empty()) continue;
          std::memset(rows, 0xff, w * 4);
          std::memcpy(rows, row.data(), row.size() * 4);
          rows += w;
        }
      });
    };
    HIPCHK(arena_stage(ar, g->device, stage));
    HIPCHK(flush(ar));
    launch_kf_scatter(ar->stream, g->kd, (int)n, dKf, dLen, dRowOf, dRows);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ar->stream));  // the arena is begun anew by the next chunk
  }
  h.kf_rows_flushed();
  return ORBFE_OK;
}

// what every call that reads the key-frame rows on the device starts with (the handle locked, the rows enabled): the
// observation table first -- the point records are there -- then the rows' own slab and their marked rows
int kf_ready(orbfe_obsgraph* g) {
  if (int rc = obs_ready(g)) return rc;
  ObsGraphMirror& h = g->h;
  if (!g->kfTable.p) {
    auto al = [](size_t x) { return (x + 255) & ~(size_t)255; };  // each of the slab's two arrays starts a line
    const size_t oLen = al((size_t)h.kfCap * h.kfRowWidth * 4), total = oLen + al((size_t)h.kfCap * 4);
    Arena* ar = &g->arena;
    int32_t* lens;
    auto stage = [&](Arena* a) -> hipError_t {
      return up_pack(a, &lens, (size_t)h.kfCap, [&](int32_t* len) {
        for (int k = 0; k < h.kfCap; k++) len[k] = (int32_t)h.kfRows[(size_t)k].size();
      });
    };
    HIPCHK(arena_stage(ar, g->device, stage));
    Slab s;
    HIPCHK(slab_get(g->device, total, &s));
    int32_t* rows = static_cast<int32_t*>(s.p);
    int32_t* len = rows + oLen / 4;
    hipError_t e = send(ar, len, lens, (size_t)h.kfCap);
    if (e == hipSuccess) e = hipStreamSynchronize(ar->stream);
    if (e != hipSuccess) { slab_put(&s); HIPCHK(e); }
    g->kfTable = s;
    g->kd.rows = rows;
    g->kd.len = len;
    g->kd.width = h.kfRowWidth;
    h.mark_kf_rows_held();
  }
  return h.dirtyKfRows.empty() ? ORBFE_OK : kf_flush(g);
}

// one group of queries [q0, q1): upload, five launches, the counts and lists back
int union_group(orbfe_obsgraph* g, int q0, int q1, const int32_t* off, const int32_t* kfs, const std::vector<int64_t>& blkOff, int capacity,
                int capDev, int32_t* slot_out, int32_t* count, bool* over) {
  const size_t Q = (size_t)(q1 - q0), nk = (size_t)(off[q1] - off[q0]), nBlocks = (size_t)(blkOff[(size_t)q1] - blkOff[(size_t)q0]);
  const size_t cap = (size_t)capDev, P = (size_t)g->h.pointCap;
  Arena* ar = &g->arena;
  int32_t *dOff, *dBlk, *dKf;
  KfUnionArgs a;
  a.nQueries = (int)Q; a.nBlocks = (int)nBlocks; a.capacity = capDev;
  auto stage = [&](Arena* s) -> hipError_t {
    TRY(up_pack(s, &dOff, Q + 1, [&](int32_t* o) {
      for (size_t q = 0; q <= Q; q++) o[q] = off[(size_t)q0 + q] - off[q0];
    }));
    TRY(up_pack(s, &dBlk, Q + 1, [&](int32_t* o) {
      for (size_t q = 0; q <= Q; q++) o[q] = (int32_t)(blkOff[(size_t)q0 + q] - blkOff[(size_t)q0]);
    }));
    TRY(up(s, &dKf, kfs + off[q0], nk));
    open_span(s);
    a.count = carve<int32_t>(s, Q);
    a.out = carve<int32_t>(s, Q * cap);
    TRY(close_span(s));
    a.first = carve<int32_t>(s, Q * P);
    a.keepMask = carve<unsigned long long>(s, nBlocks * kKfChunksPerBlock);
    a.blockCount = carve<int32_t>(s, nBlocks);
    return hipSuccess;
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  a.qOff = dOff; a.qKf = dKf; a.blkOff = dBlk;
  HIPCHK(flush(ar));
  launch_kf_union(ar->stream, g->d, g->kd, a);
  HIPCHK(hipGetLastError());
  if (span_bytes(ar) <= kUnionOneCopyBytes) {
    HIPCHK(down_span(ar));
    HIPCHK(hipStreamSynchronize(ar->stream));
  } else {
    HIPCHK(down_range(ar, a.count, a.count + Q));
    HIPCHK(hipStreamSynchronize(ar->stream));
    const int32_t* ns = mirror_of(ar, a.count);
    size_t filled = 0;  // entries up to the end of the last list that holds something
    for (size_t q = 0; q < Q; q++)
      if (ns[q] > 0) filled = q * cap + std::min((size_t)ns[q], cap);
    if (filled) {
      HIPCHK(down_range(ar, a.out, a.out + filled));
      HIPCHK(hipStreamSynchronize(ar->stream));
    }
  }
  const int32_t *ns = mirror_of(ar, a.count), *lists = mirror_of(ar, a.out);
  for (size_t q = 0; q < Q; q++) {
    count[(size_t)q0 + q] = ns[q];
    const size_t have = (size_t)std::max(ns[q], 0), m = std::min(have, cap);  // a count never exceeds point_capacity
    *over |= have > (size_t)capacity;
    if (m) std::memcpy(slot_out + ((size_t)q0 + q) * (size_t)capacity, lists + q * cap, m * 4);
  }
  return ORBFE_OK;
}

const char* kNotEnabled = "key-frame rows are not enabled (orbfe_obsgraph_enable_keyframe_points)";

}  // namespace

int orbfe::obs_kf_ready(orbfe_obsgraph* g) { return kf_ready(g); }

extern "C" int orbfe_obsgraph_enable_keyframe_points(orbfe_obsgraph* g, int kf_row_width) {
  if (!g) return obs_invalid("obsgraph_enable_keyframe_points", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  try {
    if (const char* e = g->h.enable_keyframe_points(kf_row_width)) return obs_invalid("obsgraph_enable_keyframe_points", e);
  } catch (const std::bad_alloc&) {
    return fail(ORBFE_ERR_NOMEM, "out of memory");
  }
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_set_keyframe_points(orbfe_obsgraph* g, int kf_slot, int n, const int32_t* slot) {
  if (!g) return obs_invalid("obsgraph_set_keyframe_points", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.set_keyframe_points(kf_slot, n, slot)) return obs_invalid("obsgraph_set_keyframe_points", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_assign_keyframe_points(orbfe_obsgraph* g, int n, const int32_t* kf_slot, const uint16_t* idx,
                                                     const int32_t* slot) {
  if (!g) return obs_invalid("obsgraph_assign_keyframe_points", "NULL graph");
  std::lock_guard<std::mutex> lk(g->m);
  if (const char* e = g->h.assign_keyframe_points(n, kf_slot, idx, slot)) return obs_invalid("obsgraph_assign_keyframe_points", e);
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_get_keyframe_points(orbfe_obsgraph* g, int from_device, int kf_slot, int32_t* slots, int32_t* n) {
  const char* fn = "obsgraph_get_keyframe_points";
  if (!g || !slots || !n) return obs_invalid(fn, "NULL argument");
  std::lock_guard<std::mutex> lk(g->m);
  if (!g->h.kfRowWidth) return obs_invalid(fn, kNotEnabled);
  if (kf_slot < 0 || kf_slot >= g->h.kfCap) return obs_invalid(fn, "kf slot outside [0, kf_capacity)");
  const size_t w = (size_t)g->h.kfRowWidth;
  std::memset(slots, 0xff, w * 4);  // -1 past the row's length
  if (!from_device) {
    const std::vector<int32_t>& r = g->h.kfRows[(size_t)kf_slot];
    if (!r.empty()) std::memcpy(slots, r.data(), r.size() * 4);
    *n = (int32_t)r.size();
    return ORBFE_OK;
  }
  if (int rc = kf_ready(g)) return rc;
  Arena* ar = &g->arena;
  int32_t *hLen, *hRow;
  auto stage = [&](Arena* a) { open_span(a); hLen = carve<int32_t>(a, 1); hRow = carve<int32_t>(a, w); return close_span(a); };
  HIPCHK(arena_stage(ar, g->device, stage));
  HIPCHK(fetch(ar, hLen, g->kd.len + kf_slot, 1));
  HIPCHK(fetch(ar, hRow, g->kd.rows + (size_t)kf_slot * w, w));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const int32_t len = *mirror_of(ar, hLen);
  const int live = std::min(std::max(len, 0), (int)w);
  if (live) std::memcpy(slots, mirror_of(ar, hRow), (size_t)live * 4);
  *n = len;
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_keyframe_points_union(orbfe_obsgraph* g, int n_queries, const int32_t* q_offsets, const int32_t* q_kf_slots,
                                                    int capacity, int32_t* slot_out, int32_t* count) {
  const char* fn = "obsgraph_keyframe_points_union";
  if (!g || n_queries < 0 || capacity < 0) return obs_invalid(fn, "bad argument");
  std::lock_guard<std::mutex> lk(g->m);
  if (!g->h.kfRowWidth) return obs_invalid(fn, kNotEnabled);
  if (n_queries == 0) return ORBFE_OK;
  if (n_queries > 65535) return obs_invalid(fn, "at most 65535 queries per call");
  if (!q_offsets || !count || (capacity > 0 && !slot_out)) return obs_invalid(fn, "NULL argument");
  if (const char* e = g->h.check_kf_queries(n_queries, q_offsets, q_kf_slots)) return obs_invalid(fn, e);
  if (int rc = kf_ready(g)) return rc;
  const int Q = n_queries, capDev = std::min(capacity, g->h.pointCap);  // a list never holds more than every point slot
  const size_t w = (size_t)g->h.kfRowWidth, P = (size_t)g->h.pointCap;
  std::vector<int64_t> blkOff((size_t)Q + 1, 0);
  bool over = false;
  int q0 = 0;
  size_t blocks = 0;
  for (int q = 0; q < Q; q++) {
    const size_t b = ((size_t)(q_offsets[q + 1] - q_offsets[q]) * w + kKfBlockEntries - 1) / kKfBlockEntries;
    const size_t nq = (size_t)(q - q0);
    if (nq && ((nq + 1) * P > kUnionMaxFirst || blocks + b > kUnionMaxBlocks || (nq + 1) * (size_t)capDev > kUnionMaxOut)) {
      if (int rc = union_group(g, q0, q, q_offsets, q_kf_slots, blkOff, capacity, capDev, slot_out, count, &over)) return rc;
      q0 = q;
      blocks = 0;
    }
    blocks += b;
    blkOff[(size_t)q + 1] = blkOff[(size_t)q] + (int64_t)b;  // a group's offsets are taken relative to its first query
  }
  if (int rc = union_group(g, q0, Q, q_offsets, q_kf_slots, blkOff, capacity, capDev, slot_out, count, &over)) return rc;
  if (over) return fail(ORBFE_ERR_CAPACITY, "obsgraph_keyframe_points_union: a query has more points than `capacity` (see count[])");
  return ORBFE_OK;
}

extern "C" int orbfe_obsgraph_tracked_points(orbfe_obsgraph* g, int n_kf, const int32_t* kf_slot, int min_obs, int32_t* count) {
  const char* fn = "obsgraph_tracked_points";
  if (!g || n_kf < 0) return obs_invalid(fn, "bad argument");
  std::lock_guard<std::mutex> lk(g->m);
  if (!g->h.kfRowWidth) return obs_invalid(fn, kNotEnabled);
  if (n_kf == 0) return ORBFE_OK;
  if (!kf_slot || !count) return obs_invalid(fn, "NULL argument");
  if (const char* e = g->h.check_kf_list(n_kf, kf_slot)) return obs_invalid(fn, e);
  if (int rc = kf_ready(g)) return rc;
  Arena* ar = &g->arena;
  int32_t *dKf, *dCount;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dKf, kf_slot, (size_t)n_kf));
    open_span(a);
    dCount = carve<int32_t>(a, (size_t)n_kf);
    return close_span(a);
  };
  HIPCHK(arena_stage(ar, g->device, stage));
  HIPCHK(flush(ar));
  launch_kf_tracked(ar->stream, g->d, g->kd, n_kf, dKf, min_obs, dCount);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(count, mirror_of(ar, dCount), (size_t)n_kf * 4);
  return ORBFE_OK;
}
