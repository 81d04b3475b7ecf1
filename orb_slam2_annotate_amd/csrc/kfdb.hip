// kfdb.hip -- host side of the device KeyFrameDatabase (include/orbfe.h orbfe_kfdb; kernels: k_kfdb.hip).
// Reference: src/KeyFrameDatabase.cc (add :43-49, erase :51-70, clear :72-76, DetectLoopCandidates :95-219,
// DetectRelocalizationCandidates :228-347).
//
// The BowVectors of the stored key frames live in HBM as one CSR -- words (uint32, ascending per key frame), values
// (double), and per slot (offset, count).  Slots are in list order: add() appends, so the slot index grows with the
// insertion sequence number, and erase() leaves a tombstone (count 0) that shares no word with any query; the arrays are
// compacted, order kept, once tombstones outnumber the live slots.  The three arrays grow by doubling and come from a
// pool of released slabs, so a key-frame insertion costs one small copy and never a hipMalloc / hipFree.
// The host keeps a mirror of everything it uploaded: every operand is checked on the host BEFORE it is uploaded, and
// the kernels only ever read offsets the host computed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <unordered_map>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "kfdb_kernels.h"

using namespace orbfe;

namespace {
struct HostSlot {
  int64_t id;  // the slot's index is its insertion sequence number (compaction renumbers, order kept)
  uint32_t off, n;
  bool live;
};
}  // namespace

struct orbfe_kfdb {
  int device = 0, nWords = 0;
  mutable std::mutex m;
  // host mirror
  std::vector<uint32_t> hWords;
  std::vector<double> hValues;
  std::vector<HostSlot> slots;
  std::unordered_map<int64_t, int> slotOf;  // live ids
  int nLive = 0;
  bool stale = false;  // a compaction failed half-way: the device arrays must be rewritten before they are read again
  // device CSR: slabs of the pool that the resident frames use (host_internal.h), so a released database's arrays serve
  // the next database / the next doubling
  Slab dWords, dValues, dSlots;
  // the handle's stream (made by the first call that touches the device), and what the two query calls stage through
  Arena arena;
};

namespace {

// room for `need` bytes in *s, contents [0, used) kept: a doubled slab from the pool, one device-to-device copy
int slab_reserve(orbfe_kfdb* db, Slab* s, size_t need, size_t used) {
  if (need <= s->cap) return ORBFE_OK;
  size_t want = s->cap ? s->cap : (size_t)1 << 16;
  while (want < need) want *= 2;
  Slab n;
  HIPCHK(slab_get(db->device, want, &n));
  if (used) {
    hipError_t e = hipMemcpyAsync(n.p, s->p, used, hipMemcpyDeviceToDevice, db->arena.stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->arena.stream);
    if (e != hipSuccess) { slab_put(&n); HIPCHK(e); }
  }
  slab_put(s);
  *s = n;
  return ORBFE_OK;
}

KfdbStore store_of(const orbfe_kfdb* db) {
  KfdbStore st;
  st.words = (const uint32_t*)db->dWords.p; st.values = (const double*)db->dValues.p;
  st.slots = (const KfdbSlot*)db->dSlots.p; st.nSlots = (int)db->slots.size();
  return st;
}

// drops the tombstones, order kept, and uploads everything again (amortised over the erases that made them)
int kfdb_compact(orbfe_kfdb* db) {
  std::vector<uint32_t> w; std::vector<double> v; std::vector<HostSlot> s;
  w.reserve(db->hWords.size()); v.reserve(db->hValues.size()); s.reserve((size_t)db->nLive);
  std::vector<KfdbSlot> rec;
  for (const HostSlot& h : db->slots) {
    if (!h.live) continue;
    HostSlot n = h;
    n.off = (uint32_t)w.size();
    w.insert(w.end(), db->hWords.begin() + h.off, db->hWords.begin() + h.off + h.n);
    v.insert(v.end(), db->hValues.begin() + h.off, db->hValues.begin() + h.off + h.n);
    s.push_back(n);
    rec.push_back({n.off, n.n});
  }
  // (the slabs only ever grow, so everything fits)
  if (!w.empty()) {
    HIPCHK(hipMemcpyAsync(db->dWords.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, db->arena.stream));
    HIPCHK(hipMemcpyAsync(db->dValues.p, v.data(), v.size() * 8, hipMemcpyHostToDevice, db->arena.stream));
  }
  if (!rec.empty()) HIPCHK(hipMemcpyAsync(db->dSlots.p, rec.data(), rec.size() * sizeof(KfdbSlot), hipMemcpyHostToDevice, db->arena.stream));
  HIPCHK(hipStreamSynchronize(db->arena.stream));
  db->stale = false;
  db->hWords.swap(w); db->hValues.swap(v); db->slots.swap(s);
  db->slotOf.clear();
  for (size_t i = 0; i < db->slots.size(); i++) db->slotOf[db->slots[i].id] = (int)i;
  return ORBFE_OK;
}

// what every call that reads or writes the device arrays starts with
int kfdb_ready(orbfe_kfdb* db) {
  HIPCHK(arena_stream(&db->arena, db->device));
  return db->stale ? kfdb_compact(db) : ORBFE_OK;
}

// a BowVector as the caller gives it: ids ascending and unique, all below n_words
bool bow_ok(const uint32_t* w, int n, int nWords) {
  for (int i = 0; i < n; i++)
    if (w[i] >= (uint32_t)nWords || (i > 0 && w[i] <= w[i - 1])) return false;
  return true;
}

}  // namespace

extern "C" int orbfe_kfdb_create(int n_words, int device, orbfe_kfdb** out) {
  if (!out) return fail(ORBFE_ERR_INVALID, "kfdb_create: NULL argument");
  *out = nullptr;
  if (n_words <= 0 || device < 0) return fail(ORBFE_ERR_INVALID, "kfdb_create: n_words must be positive, device non-negative");
  orbfe_kfdb* db = new (std::nothrow) orbfe_kfdb();
  if (!db) return fail(ORBFE_ERR_NOMEM, "out of memory");
  db->device = device; db->nWords = n_words;
  *out = db;  // the device is first touched by the call that uploads something
  return ORBFE_OK;
}

extern "C" void orbfe_kfdb_destroy(orbfe_kfdb* db) {
  if (!db) return;
  if (db->arena.stream) {
    (void)hipSetDevice(db->device);
    (void)hipStreamSynchronize(db->arena.stream);
    slab_put(&db->dWords);
    slab_put(&db->dValues);
    slab_put(&db->dSlots);
  }
  delete db;  // (the arena's end: the stream, then the buffers)
}

extern "C" int orbfe_kfdb_size(const orbfe_kfdb* db) {
  if (!db) return fail(ORBFE_ERR_INVALID, "NULL kfdb");
  std::lock_guard<std::mutex> lk(db->m);
  return db->nLive;
}

extern "C" int orbfe_kfdb_add(orbfe_kfdb* db, int64_t kf_id, const uint32_t* word_ids, const double* values, int n) {
  if (!db || n < 0 || (n > 0 && (!word_ids || !values))) return fail(ORBFE_ERR_INVALID, "kfdb_add: bad argument");
  std::lock_guard<std::mutex> lk(db->m);
  if (db->slotOf.count(kf_id)) return fail(ORBFE_ERR_INVALID, "kfdb_add: key frame id already in the database");
  if (!bow_ok(word_ids, n, db->nWords))
    return fail(ORBFE_ERR_INVALID, "kfdb_add: word ids must ascend strictly and stay below n_words");
  if (db->hWords.size() + (size_t)n > 0xffffffffull) return fail(ORBFE_ERR_CAPACITY, "kfdb_add: more than 2^32 stored words");
  int rc;
  if ((rc = kfdb_ready(db))) return rc;
  const size_t used = db->hWords.size(), nSlots = db->slots.size();
  if ((rc = slab_reserve(db, &db->dWords, (used + n) * 4, used * 4))) return rc;
  if ((rc = slab_reserve(db, &db->dValues, (used + n) * 8, used * 8))) return rc;
  if ((rc = slab_reserve(db, &db->dSlots, (nSlots + 1) * sizeof(KfdbSlot), nSlots * sizeof(KfdbSlot)))) return rc;
  const KfdbSlot rec = {(uint32_t)used, (uint32_t)n};
  if (n) {
    HIPCHK(hipMemcpyAsync((uint32_t*)db->dWords.p + used, word_ids, (size_t)n * 4, hipMemcpyHostToDevice, db->arena.stream));
    HIPCHK(hipMemcpyAsync((double*)db->dValues.p + used, values, (size_t)n * 8, hipMemcpyHostToDevice, db->arena.stream));
  }
  HIPCHK(hipMemcpyAsync((KfdbSlot*)db->dSlots.p + nSlots, &rec, sizeof rec, hipMemcpyHostToDevice, db->arena.stream));
  HIPCHK(hipStreamSynchronize(db->arena.stream));
  // the device holds it: commit to the mirror
  db->hWords.insert(db->hWords.end(), word_ids, word_ids + n);
  db->hValues.insert(db->hValues.end(), values, values + n);
  db->slots.push_back({kf_id, rec.off, rec.n, true});
  db->slotOf[kf_id] = (int)nSlots;
  db->nLive++;
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_erase(orbfe_kfdb* db, int64_t kf_id) {
  if (!db) return fail(ORBFE_ERR_INVALID, "NULL kfdb");
  std::lock_guard<std::mutex> lk(db->m);
  auto it = db->slotOf.find(kf_id);
  if (it == db->slotOf.end()) return 0;  // the reference's erase of an absent key frame finds nothing to remove
  int rc;
  if ((rc = kfdb_ready(db))) return rc;
  const int s = it->second;
  const KfdbSlot rec = {db->slots[(size_t)s].off, 0u};
  HIPCHK(hipMemcpyAsync((KfdbSlot*)db->dSlots.p + s, &rec, sizeof rec, hipMemcpyHostToDevice, db->arena.stream));
  HIPCHK(hipStreamSynchronize(db->arena.stream));
  db->slots[(size_t)s].live = false;
  db->slotOf.erase(it);
  db->nLive--;
  const int dead = (int)db->slots.size() - db->nLive;
  // The erase is committed.  A compaction that fails may have rewritten part of the device arrays: the mirror (swapped
  // only after the uploads have completed) stays the truth, and the next call rewrites the arrays from it or fails.
  if (dead > 32 && dead > db->nLive && kfdb_compact(db)) db->stale = true;
  return 1;
}

extern "C" int orbfe_kfdb_clear(orbfe_kfdb* db) {
  if (!db) return fail(ORBFE_ERR_INVALID, "NULL kfdb");
  std::lock_guard<std::mutex> lk(db->m);
  db->hWords.clear(); db->hValues.clear(); db->slots.clear(); db->slotOf.clear();
  db->nLive = 0;  // the slabs stay with the handle
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_query(orbfe_kfdb* db, int n_queries, const int32_t* q_offsets, const uint32_t* q_words,
                                const double* q_values, const int32_t* excl_offsets, const int64_t* excl_ids, int capacity,
                                int64_t* kf_id, int32_t* n_common, float* score, int32_t* count) {
  if (!db || n_queries < 0 || capacity < 0) return fail(ORBFE_ERR_INVALID, "kfdb_query: bad argument");
  if (n_queries == 0) return ORBFE_OK;
  if (n_queries > 65535) return fail(ORBFE_ERR_INVALID, "kfdb_query: at most 65535 queries per call");  // the grid's y extent
  if (!q_offsets || !count || (capacity > 0 && (!kf_id || !n_common || !score)))
    return fail(ORBFE_ERR_INVALID, "kfdb_query: NULL argument");
  const int Q = n_queries;
  if (q_offsets[0] != 0) return fail(ORBFE_ERR_INVALID, "kfdb_query: q_offsets[0] must be 0");
  int maxWords = 0;
  for (int q = 0; q < Q; q++) {
    const int n = q_offsets[q + 1] - q_offsets[q];
    if (n < 0 || (n > 0 && (!q_words || !q_values))) return fail(ORBFE_ERR_INVALID, "kfdb_query: q_offsets must not descend");
    if (!bow_ok(q_words + q_offsets[q], n, db->nWords))
      return fail(ORBFE_ERR_INVALID, "kfdb_query: word ids must ascend strictly and stay below n_words");
    maxWords = std::max(maxWords, n);
  }
  const size_t nq = (size_t)q_offsets[Q];
  size_t nExcl = 0;
  if (excl_offsets) {
    if (excl_offsets[0] != 0) return fail(ORBFE_ERR_INVALID, "kfdb_query: excl_offsets[0] must be 0");
    for (int q = 0; q < Q; q++)
      if (excl_offsets[q + 1] < excl_offsets[q]) return fail(ORBFE_ERR_INVALID, "kfdb_query: excl_offsets must not descend");
    nExcl = (size_t)excl_offsets[Q];
    if (nExcl && !excl_ids) return fail(ORBFE_ERR_INVALID, "kfdb_query: NULL excl_ids");
  }
  std::lock_guard<std::mutex> lk(db->m);
  int rc;
  if ((rc = kfdb_ready(db))) return rc;
  if (db->nLive == 0) {
    for (int q = 0; q < Q; q++) count[q] = 0;
    return ORBFE_OK;
  }
  const size_t N = db->slots.size(), cap = (size_t)capacity, nQ = (size_t)Q;
  // ids -> slots, packed in place (either array, or none: the count); an id the database does not hold excludes nothing
  auto excluded = [&](int32_t* off, uint32_t* slots) {
    int nx = 0;
    for (int q = 0; q <= Q; q++) {
      if (off) off[q] = nx;
      if (q == Q || !excl_offsets) continue;
      for (int i = excl_offsets[q]; i < excl_offsets[q + 1]; i++) {
        auto it = db->slotOf.find(excl_ids[i]);
        if (it == db->slotOf.end()) continue;
        if (slots) slots[nx] = (uint32_t)it->second;
        nx++;
      }
    }
    return nx;
  };
  Arena* ar = &db->arena;
  KfdbQueries p = {};
  p.maxWords = maxWords;
  p.capacity = capacity;
  int32_t *dOff, *dExOff;
  uint32_t *dWords, *dExSlots;
  double* dValues;
  // (the three Q x slots work arrays grow per key frame; the arena grows by half and 1 MB, so a regrow stays rare)
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dOff, q_offsets, nQ + 1));
    TRY(up_pack(a, &dExOff, nQ + 1, [&](int32_t* off) { p.nExcl = excluded(off, nullptr); }));
    TRY(up(a, &dWords, q_words, nq));
    TRY(up_pack(a, &dExSlots, nExcl, [&](uint32_t* slots) { excluded(nullptr, slots); }));
    TRY(up(a, &dValues, q_values, nq));
    open_span(a);
    p.nSurv = carve<int32_t>(a, nQ);
    p.outSlot = carve<uint32_t>(a, nQ * cap);
    p.outCommon = carve<int32_t>(a, nQ * cap);
    p.outScore = carve<float>(a, nQ * cap);
    TRY(close_span(a));
    p.common = carve<uint32_t>(a, nQ * N);
    p.minWord = carve<uint32_t>(a, nQ * N);
    p.surv = carve<uint32_t>(a, nQ * N);
    return hipSuccess;
  };
  HIPCHK(arena_stage(ar, db->device, stage));
  p.qOff = dOff; p.qWords = dWords; p.qValues = dValues;
  p.exclOff = dExOff; p.exclSlots = dExSlots;
  HIPCHK(flush(ar));
  launch_kfdb_query(ar->stream, store_of(db), p, Q);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const int32_t *ns = mirror_of(ar, p.nSurv), *hCommon = mirror_of(ar, p.outCommon);
  const uint32_t* os = mirror_of(ar, p.outSlot);
  const float* hScore = mirror_of(ar, p.outScore);
  bool over = false;
  for (int q = 0; q < Q; q++) {
    count[q] = ns[q];
    const size_t m = std::min((size_t)ns[q], cap);
    over |= (size_t)ns[q] > cap;
    for (size_t i = 0; i < m; i++) {
      const uint32_t s = os[q * cap + i];
      kf_id[q * cap + i] = s < N ? db->slots[s].id : -1;
    }
    if (m) {
      memcpy(n_common + q * cap, hCommon + q * cap, m * 4);
      memcpy(score + q * cap, hScore + q * cap, m * 4);
    }
  }
  if (over) return fail(ORBFE_ERR_CAPACITY, "kfdb_query: a query has more scored key frames than `capacity` (see count[])");
  return ORBFE_OK;
}

extern "C" int orbfe_kfdb_score(orbfe_kfdb* db, const uint32_t* q_words, const double* q_values, int n, int n_ids,
                                const int64_t* kf_ids, double* scores) {
  if (!db || n < 0 || n_ids < 0 || (n > 0 && (!q_words || !q_values)) || (n_ids > 0 && (!kf_ids || !scores)))
    return fail(ORBFE_ERR_INVALID, "kfdb_score: bad argument");
  if (!bow_ok(q_words, n, db->nWords))
    return fail(ORBFE_ERR_INVALID, "kfdb_score: word ids must ascend strictly and stay below n_words");
  if (n_ids == 0) return ORBFE_OK;
  std::lock_guard<std::mutex> lk(db->m);
  std::vector<uint32_t> slotIds((size_t)n_ids);
  for (int i = 0; i < n_ids; i++) {
    auto it = db->slotOf.find(kf_ids[i]);
    if (it == db->slotOf.end()) return fail(ORBFE_ERR_INVALID, "kfdb_score: key frame id not in the database");
    slotIds[(size_t)i] = (uint32_t)it->second;
  }
  int rc;
  if ((rc = kfdb_ready(db))) return rc;
  Arena* ar = &db->arena;
  const int32_t off[2] = {0, n};
  int32_t* dOff;
  uint32_t *dWords, *dSlotIds;
  double *dValues, *dScores;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &dOff, off, 2));
    TRY(up(a, &dWords, q_words, (size_t)n));
    TRY(up(a, &dSlotIds, slotIds.data(), (size_t)n_ids));
    TRY(up(a, &dValues, q_values, (size_t)n));
    open_span(a);
    dScores = carve<double>(a, (size_t)n_ids);
    return close_span(a);
  };
  HIPCHK(arena_stage(ar, db->device, stage));
  HIPCHK(flush(ar));
  KfdbQueries p = {};
  p.qOff = dOff; p.qWords = dWords; p.qValues = dValues;
  p.maxWords = n;
  launch_kfdb_score(ar->stream, store_of(db), p, dSlotIds, n_ids, dScores);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  memcpy(scores, mirror_of(ar, dScores), (size_t)n_ids * 8);
  return ORBFE_OK;
}

// The covisibility stage of both Detect*Candidates (:165-218, :293-346) over one query's scored set.  Pure host code.
extern "C" int orbfe_kfdb_group_candidates(int mode, float min_score, int n, const int64_t* kf_id, const int32_t* n_common,
                                           const float* score, const int32_t* neigh_offsets, const int64_t* neigh_ids,
                                           int64_t* out_ids, int capacity, int* n_out) {
  (void)n_common;  // every entry of the scored set has passed the word-count filter already
  if ((mode != ORBFE_KFDB_RELOC && mode != ORBFE_KFDB_LOOP) || n < 0 || capacity < 0 || !n_out ||
      (n > 0 && (!kf_id || !score || !neigh_offsets)) || (capacity > 0 && !out_ids))
    return fail(ORBFE_ERR_INVALID, "kfdb_group_candidates: bad argument");
  *n_out = 0;
  if (n == 0) return ORBFE_OK;
  if (neigh_offsets[0] != 0) return fail(ORBFE_ERR_INVALID, "kfdb_group_candidates: neigh_offsets[0] must be 0");
  for (int i = 0; i < n; i++)
    if (neigh_offsets[i + 1] < neigh_offsets[i]) return fail(ORBFE_ERR_INVALID, "kfdb_group_candidates: neigh_offsets must not descend");
  if (neigh_offsets[n] > 0 && !neigh_ids) return fail(ORBFE_ERR_INVALID, "kfdb_group_candidates: NULL neigh_ids");
  std::unordered_map<int64_t, int> scored;  // mnLoopQuery / mnRelocQuery == the query's id, and a score that was computed
  for (int i = 0; i < n; i++) scored.emplace(kf_id[i], i);
  const bool loop = mode == ORBFE_KFDB_LOOP;
  std::vector<std::pair<float, int64_t>> acc;  // lAccScoreAndMatch
  float bestAccScore = loop ? min_score : 0.0f;
  for (int i = 0; i < n; i++) {
    if (loop && !(score[i] >= min_score)) continue;  // lScoreAndMatch holds si >= minScore only (:157)
    float bestScore = score[i], accScore = score[i];
    int64_t best = kf_id[i];
    for (int j = neigh_offsets[i]; j < neigh_offsets[i + 1]; j++) {
      auto it = scored.find(neigh_ids[j]);
      if (it == scored.end()) continue;
      const float s2 = score[it->second];
      accScore += s2;
      if (s2 > bestScore) { best = neigh_ids[j]; bestScore = s2; }
    }
    acc.emplace_back(accScore, best);
    if (accScore > bestAccScore) bestAccScore = accScore;
  }
  const float minScoreToRetain = 0.75f * bestAccScore;
  std::vector<int64_t> out;
  for (const auto& a : acc) {
    if (!(a.first > minScoreToRetain)) continue;
    if (std::find(out.begin(), out.end(), a.second) != out.end()) continue;  // spAlreadyAddedKF
    out.push_back(a.second);
  }
  *n_out = (int)out.size();
  const size_t m = std::min(out.size(), (size_t)capacity);
  if (m) memcpy(out_ids, out.data(), m * sizeof(int64_t));
  if (out.size() > (size_t)capacity) return fail(ORBFE_ERR_CAPACITY, "kfdb_group_candidates: more candidates than `capacity` (see n_out)");
  return ORBFE_OK;
}
