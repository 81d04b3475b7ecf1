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
  bool ready = false;  // stream created
  hipStream_t stream = nullptr;
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
  // grow-only workspace of the queries + pinned staging in both directions
  DevBuf<uint8_t> work;
  PinBuf<uint8_t> pin;
};

namespace {

int kfdb_device(orbfe_kfdb* db) {
  HIPCHK(hipSetDevice(db->device));
  if (!db->ready) {
    HIPCHK(hipStreamCreateWithFlags(&db->stream, hipStreamNonBlocking));
    db->ready = true;
  }
  return ORBFE_OK;
}

// `have` (or `first` when there is nothing yet), doubled until it holds `need`
size_t doubled(size_t have, size_t first, size_t need) {
  size_t want = have ? have : first;
  while (want < need) want *= 2;
  return want;
}

// room for `need` bytes in *s, contents [0, used) kept: a doubled slab from the pool, one device-to-device copy
int slab_reserve(orbfe_kfdb* db, Slab* s, size_t need, size_t used) {
  if (need <= s->cap) return ORBFE_OK;
  Slab n;
  HIPCHK(slab_get(db->device, doubled(s->cap, (size_t)1 << 16, need), &n));
  if (used) {
    hipError_t e = hipMemcpyAsync(n.p, s->p, used, hipMemcpyDeviceToDevice, db->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(db->stream);
    if (e != hipSuccess) { slab_put(&n); HIPCHK(e); }
  }
  slab_put(s);
  *s = n;
  return ORBFE_OK;
}

int ensure_work(orbfe_kfdb* db, size_t devBytes, size_t pinBytes) {
  const int rc = db->work.reserve(devBytes, doubled(db->work.cap, (size_t)1 << 20, devBytes));
  return rc ? rc : db->pin.reserve(pinBytes, doubled(db->pin.cap, (size_t)1 << 16, pinBytes));
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
    HIPCHK(hipMemcpyAsync(db->dWords.p, w.data(), w.size() * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync(db->dValues.p, v.data(), v.size() * 8, hipMemcpyHostToDevice, db->stream));
  }
  if (!rec.empty()) HIPCHK(hipMemcpyAsync(db->dSlots.p, rec.data(), rec.size() * sizeof(KfdbSlot), hipMemcpyHostToDevice, db->stream));
  HIPCHK(hipStreamSynchronize(db->stream));
  db->stale = false;
  db->hWords.swap(w); db->hValues.swap(v); db->slots.swap(s);
  db->slotOf.clear();
  for (size_t i = 0; i < db->slots.size(); i++) db->slotOf[db->slots[i].id] = (int)i;
  return ORBFE_OK;
}

// what every call that reads or writes the device arrays starts with
int kfdb_ready(orbfe_kfdb* db) {
  int rc = kfdb_device(db);
  if (!rc && db->stale) rc = kfdb_compact(db);
  return rc;
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
  if (db->ready) {
    (void)hipSetDevice(db->device);
    (void)hipStreamSynchronize(db->stream);
    slab_put(&db->dWords);
    slab_put(&db->dValues);
    slab_put(&db->dSlots);
    (void)hipStreamDestroy(db->stream);
  }
  delete db;
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
    HIPCHK(hipMemcpyAsync((uint32_t*)db->dWords.p + used, word_ids, (size_t)n * 4, hipMemcpyHostToDevice, db->stream));
    HIPCHK(hipMemcpyAsync((double*)db->dValues.p + used, values, (size_t)n * 8, hipMemcpyHostToDevice, db->stream));
  }
  HIPCHK(hipMemcpyAsync((KfdbSlot*)db->dSlots.p + nSlots, &rec, sizeof rec, hipMemcpyHostToDevice, db->stream));
  HIPCHK(hipStreamSynchronize(db->stream));
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
  HIPCHK(hipMemcpyAsync((KfdbSlot*)db->dSlots.p + s, &rec, sizeof rec, hipMemcpyHostToDevice, db->stream));
  HIPCHK(hipStreamSynchronize(db->stream));
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

namespace {
size_t align16(size_t x) { return (x + 15) & ~(size_t)15; }
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
  const size_t N = db->slots.size(), cap = (size_t)capacity;
  // upload block: qOff | exclOff | qWords | exclSlots | qValues     download block: nSurv | outSlot | outCommon | outScore
  const size_t uOff = 0, uEx = align16(uOff + (Q + 1) * 4), uW = align16(uEx + (Q + 1) * 4), uXs = align16(uW + nq * 4),
               uV = align16(uXs + nExcl * 4), upBytes = align16(uV + nq * 8);
  const size_t oN = 0, oS = align16(oN + (size_t)Q * 4), oC = align16(oS + Q * cap * 4), oF = align16(oC + Q * cap * 4),
               downBytes = align16(oF + Q * cap * 4);
  const size_t wCommon = upBytes, wMin = wCommon + align16(Q * N * 4), wSurv = wMin + align16(Q * N * 4),
               wOut = wSurv + align16(Q * N * 4);
  // sized by the slot slab's capacity (>= N), so that the workspace doubles with the database instead of growing per key frame
  const size_t slotCap = db->dSlots.cap / sizeof(KfdbSlot);
  const size_t devBytes = upBytes + 3 * align16(Q * slotCap * 4) + downBytes;
  if ((rc = ensure_work(db, devBytes, std::max(upBytes, downBytes)))) return rc;
  uint8_t* h = db->pin;
  uint8_t* d = db->work;
  memcpy(h + uOff, q_offsets, (size_t)(Q + 1) * 4);
  int32_t* hEx = (int32_t*)(h + uEx);
  uint32_t* hXs = (uint32_t*)(h + uXs);
  size_t nx = 0;
  for (int q = 0; q < Q; q++) {  // ids -> slots; an id the database does not hold excludes nothing
    hEx[q] = (int32_t)nx;
    if (excl_offsets)
      for (int i = excl_offsets[q]; i < excl_offsets[q + 1]; i++) {
        auto it = db->slotOf.find(excl_ids[i]);
        if (it != db->slotOf.end()) hXs[nx++] = (uint32_t)it->second;
      }
  }
  hEx[Q] = (int32_t)nx;
  if (nq) {
    memcpy(h + uW, q_words, nq * 4);
    memcpy(h + uV, q_values, nq * 8);
  }
  HIPCHK(hipMemcpyAsync(d, h, upBytes, hipMemcpyHostToDevice, db->stream));
  KfdbQueries p = {};
  p.qOff = (const int32_t*)(d + uOff); p.qWords = (const uint32_t*)(d + uW); p.qValues = (const double*)(d + uV);
  p.maxWords = maxWords;
  p.exclOff = (const int32_t*)(d + uEx); p.exclSlots = (const uint32_t*)(d + uXs); p.nExcl = (int)nx;
  p.common = (uint32_t*)(d + wCommon); p.minWord = (uint32_t*)(d + wMin); p.surv = (uint32_t*)(d + wSurv);
  p.nSurv = (int32_t*)(d + wOut + oN);
  p.capacity = capacity;
  p.outSlot = (uint32_t*)(d + wOut + oS); p.outCommon = (int32_t*)(d + wOut + oC); p.outScore = (float*)(d + wOut + oF);
  launch_kfdb_query(db->stream, store_of(db), p, Q);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, d + wOut, downBytes, hipMemcpyDeviceToHost, db->stream));
  HIPCHK(hipStreamSynchronize(db->stream));
  const int32_t* ns = (const int32_t*)(h + oN);
  const uint32_t* os = (const uint32_t*)(h + oS);
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
      memcpy(n_common + q * cap, h + oC + q * cap * 4, m * 4);
      memcpy(score + q * cap, h + oF + q * cap * 4, m * 4);
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
  const size_t uOff = 0, uW = 16, uS = align16(uW + (size_t)n * 4), uV = align16(uS + (size_t)n_ids * 4),
               upBytes = align16(uV + (size_t)n * 8), downBytes = (size_t)n_ids * 8;
  if ((rc = ensure_work(db, upBytes + downBytes, std::max(upBytes, downBytes)))) return rc;
  uint8_t* h = db->pin;
  uint8_t* d = db->work;
  const int32_t off[2] = {0, n};
  memcpy(h + uOff, off, sizeof off);
  if (n) {
    memcpy(h + uW, q_words, (size_t)n * 4);
    memcpy(h + uV, q_values, (size_t)n * 8);
  }
  memcpy(h + uS, slotIds.data(), (size_t)n_ids * 4);
  HIPCHK(hipMemcpyAsync(d, h, upBytes, hipMemcpyHostToDevice, db->stream));
  KfdbQueries p = {};
  p.qOff = (const int32_t*)(d + uOff); p.qWords = (const uint32_t*)(d + uW); p.qValues = (const double*)(d + uV);
  p.maxWords = n;
  launch_kfdb_score(db->stream, store_of(db), p, (const uint32_t*)(d + uS), n_ids, (double*)(d + upBytes));
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(h, d + upBytes, downBytes, hipMemcpyDeviceToHost, db->stream));
  HIPCHK(hipStreamSynchronize(db->stream));
  memcpy(scores, h, downBytes);
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
