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

size_t al(size_t x) { return obs_al(x); }

// the marked key-frame rows onto the device; the marks are dropped only when everything has arrived
int kf_flush(orbfe_obsgraph* g) {
  ObsGraphMirror& h = g->h;
  const size_t w = (size_t)h.kfRowWidth;
  const size_t perRow = 12 + w * 4;
  const size_t rowsPerChunk = std::max<size_t>(1, kObsFlushChunkBytes / perRow);
  for (size_t at = 0; at < h.dirtyKfRows.size(); at += rowsPerChunk) {
    const size_t n = std::min(rowsPerChunk, h.dirtyKfRows.size() - at);
    const size_t oKf = 0, oLen = al(oKf + n * 4), oRowOf = al(oLen + n * 4), oRows = al(oRowOf + n * 4);
    size_t nRows = 0;
    for (size_t i = 0; i < n; i++) nRows += !h.kfRows[(size_t)h.dirtyKfRows[at + i]].empty();
    const size_t bytes = al(oRows + nRows * w * 4);
    if (int rc = obs_ensure_work(g, bytes, bytes)) return rc;
    uint8_t* p = g->pin;
    uint8_t* d = g->work;
    int32_t *hKf = (int32_t*)(p + oKf), *hLen = (int32_t*)(p + oLen), *hRowOf = (int32_t*)(p + oRowOf), *hRows = (int32_t*)(p + oRows);
    size_t r = 0;
    for (size_t i = 0; i < n; i++) {
      const int32_t k = h.dirtyKfRows[at + i];
      const std::vector<int32_t>& row = h.kfRows[(size_t)k];
      hKf[i] = k;
      hLen[i] = (int32_t)row.size();
      hRowOf[i] = row.empty() ? -1 : (int32_t)r;
      if (!row.empty()) {
        std::memset(hRows + r * w, 0xff, w * 4);
        std::memcpy(hRows + r * w, row.data(), row.size() * 4);
        r++;
      }
    }
    HIPCHK(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, g->stream));
    launch_kf_scatter(g->stream, g->kd, (int)n, (const int32_t*)(d + oKf), (const int32_t*)(d + oLen), (const int32_t*)(d + oRowOf),
                      (const int32_t*)(d + oRows));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(g->stream));  // the staging block is reused by the next chunk
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
    const size_t oLen = al((size_t)h.kfCap * h.kfRowWidth * 4), total = oLen + al((size_t)h.kfCap * 4);
    if (int rc = obs_ensure_work(g, 0, (size_t)h.kfCap * 4)) return rc;
    Slab s;
    HIPCHK(slab_get(g->device, total, &s));
    uint8_t* b = static_cast<uint8_t*>(s.p);
    uint8_t* p = g->pin;
    int32_t* lens = (int32_t*)p;
    for (int k = 0; k < h.kfCap; k++) lens[k] = (int32_t)h.kfRows[(size_t)k].size();
    hipError_t e = hipMemcpyAsync(b + oLen, lens, (size_t)h.kfCap * 4, hipMemcpyHostToDevice, g->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
    if (e != hipSuccess) { slab_put(&s); HIPCHK(e); }
    g->kfTable = s;
    g->kd.rows = reinterpret_cast<int32_t*>(b);
    g->kd.len = reinterpret_cast<int32_t*>(b + oLen);
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
  const size_t uOff = 0, uBlk = al(uOff + (Q + 1) * 4), uKf = al(uBlk + (Q + 1) * 4), upBytes = al(uKf + nk * 4);
  const size_t wFirst = upBytes, wMask = al(wFirst + Q * P * 4), wCount = al(wMask + nBlocks * kKfChunksPerBlock * 8),
               wDown = al(wCount + nBlocks * 4);
  const size_t oCount = 0, oOut = al(Q * 4), downBytes = oOut + al(Q * cap * 4);
  if (int rc = obs_ensure_work(g, wDown + downBytes, std::max(upBytes, downBytes))) return rc;
  uint8_t* p = g->pin;
  uint8_t* d = g->work;
  int32_t *hOff = (int32_t*)(p + uOff), *hBlk = (int32_t*)(p + uBlk);
  for (size_t q = 0; q <= Q; q++) {
    hOff[q] = off[(size_t)q0 + q] - off[q0];
    hBlk[q] = (int32_t)(blkOff[(size_t)q0 + q] - blkOff[(size_t)q0]);
  }
  if (nk) std::memcpy(p + uKf, kfs + off[q0], nk * 4);
  HIPCHK(hipMemcpyAsync(d, p, upBytes, hipMemcpyHostToDevice, g->stream));
  uint8_t* o = d + wDown;
  KfUnionArgs a;
  a.nQueries = (int)Q; a.nBlocks = (int)nBlocks; a.capacity = capDev;
  a.qOff = (const int32_t*)(d + uOff); a.qKf = (const int32_t*)(d + uKf); a.blkOff = (const int32_t*)(d + uBlk);
  a.first = (int32_t*)(d + wFirst); a.keepMask = (unsigned long long*)(d + wMask); a.blockCount = (int32_t*)(d + wCount);
  a.out = (int32_t*)(o + oOut); a.count = (int32_t*)(o + oCount);
  launch_kf_union(g->stream, g->d, g->kd, a);
  HIPCHK(hipGetLastError());
  const int32_t* ns = (const int32_t*)(p + oCount);
  if (downBytes <= kUnionOneCopyBytes) {
    HIPCHK(hipMemcpyAsync(p, o, downBytes, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
  } else {
    HIPCHK(hipMemcpyAsync(p, o, Q * 4, hipMemcpyDeviceToHost, g->stream));
    HIPCHK(hipStreamSynchronize(g->stream));
    size_t filled = 0;  // entries up to the end of the last list that holds something
    for (size_t q = 0; q < Q; q++)
      if (ns[q] > 0) filled = q * cap + std::min((size_t)ns[q], cap);
    if (filled) {
      HIPCHK(hipMemcpyAsync(p + oOut, o + oOut, filled * 4, hipMemcpyDeviceToHost, g->stream));
      HIPCHK(hipStreamSynchronize(g->stream));
    }
  }
  for (size_t q = 0; q < Q; q++) {
    count[(size_t)q0 + q] = ns[q];
    const size_t have = (size_t)std::max(ns[q], 0), m = std::min(have, cap);  // a count never exceeds point_capacity
    *over |= have > (size_t)capacity;
    if (m) std::memcpy(slot_out + ((size_t)q0 + q) * (size_t)capacity, p + oOut + q * cap * 4, m * 4);
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
  const size_t oRow = al(4), bytes = oRow + w * 4;
  if (int rc = obs_ensure_work(g, 0, bytes)) return rc;
  uint8_t* p = g->pin;
  HIPCHK(hipMemcpyAsync(p, g->kd.len + kf_slot, 4, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipMemcpyAsync(p + oRow, g->kd.rows + (size_t)kf_slot * w, w * 4, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  int32_t len;
  std::memcpy(&len, p, 4);
  const int live = std::min(std::max(len, 0), (int)w);
  if (live) std::memcpy(slots, p + oRow, (size_t)live * 4);
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
  const size_t bytes = al((size_t)n_kf * 4);
  if (int rc = obs_ensure_work(g, 2 * bytes, bytes)) return rc;
  uint8_t* p = g->pin;
  uint8_t* d = g->work;
  std::memcpy(p, kf_slot, (size_t)n_kf * 4);
  HIPCHK(hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, g->stream));
  launch_kf_tracked(g->stream, g->d, g->kd, n_kf, (const int32_t*)d, min_obs, (int32_t*)(d + bytes));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(p, d + bytes, bytes, hipMemcpyDeviceToHost, g->stream));
  HIPCHK(hipStreamSynchronize(g->stream));
  std::memcpy(count, p, (size_t)n_kf * 4);
  return ORBFE_OK;
}
