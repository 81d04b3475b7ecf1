// vocabulary.hip -- DBoW2 ORB vocabulary on the device: text loader (TemplatedVocabulary::
// loadFromTextFile, Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424) and transform()
// (:1127-1194 feature loop, :1218-1259 k-ary descent with FORB::distance, FORB.cpp:81-101).
// the step immediately before SearchByBoW (src/Frame.cc:433-440).
//
// The handle, the loader and the entry points; the two kernels and their launchers are k_vocab.hip.  The tree is immutable after
// create: orbfe_vocabulary_transform and orbfe_vocabulary_featvec_batch_device keep nothing on the handle -- they stage through
// the calling thread's arena and run on its stream, so several threads may call them on one handle at once (the reference does:
// Frame::ComputeBoW on tracking, KeyFrame::ComputeBoW on local mapping).  The consecutive-frame batch keeps a workspace that
// outlives the call on other streams, and with it the handle's own stream and events.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <sstream>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "kernels.h"
#include "match_kernels.h"

using namespace orbfe;

struct orbfe_vocabulary {
  int device = 0;
  int k = 0, L = 0, scoring = 0, weighting = 0;
  int nNodes = 0, nWords = 0;
  hipStream_t stream = nullptr;
  DevBuf<VocabNode> nodes; DevBuf<double> weight;  // the tree; `d` is what the kernels take of it
  VocabDevice d = {};
  // grow-only workspace of the consecutive-frame batch (bow_match_consecutive)
  DevBuf<uint32_t> w_nodes, w_indices; DevBuf<int32_t> w_offsets, w_count;
  DevBuf<int8_t> w_bin; DevBuf<unsigned long long> w_keys;
  size_t wFrames = 0; int wCap = 0;
  hipStream_t lastStream = nullptr;  // stream of the last batched call (its workspace may still be in use there)
  hipEvent_t evFv[32] = {}, evBoundary[32] = {};  // per sub-batch: FeatureVectors built / boundary pair searched
  orbfe_extractor* lastMulti = nullptr;  // extractor whose sub-batch streams ran the last per-sub-batch call
};

// the events and the stream of the handle (its buffers free themselves when it is deleted)
static void vocab_destroy_sync_objects(orbfe_vocabulary* v) {
  for (int i = 0; i < 32; i++) {
    if (v->evFv[i]) (void)hipEventDestroy(v->evFv[i]);
    if (v->evBoundary[i]) (void)hipEventDestroy(v->evBoundary[i]);
  }
  if (v->stream) (void)hipStreamDestroy(v->stream);
}

// Nodes 1..n of a DBoW2 tree as the text file lists them (node 0 = the root) -> BFS records on the device.
static int vocab_upload(orbfe_vocabulary* v, const int32_t* parent, const uint8_t* desc, const double* weight,
                        const int32_t* wordId) {
  const int n = v->nNodes;
  std::vector<int32_t> off((size_t)n + 1, 0), idx((size_t)(n > 1 ? n - 1 : 1), 0);
  for (int i = 1; i < n; i++) {
    if (parent[i] < 0 || parent[i] >= n) return fail(ORBFE_ERR_INVALID, "vocabulary: parent id out of range");
    // every descent must terminate: a child's id is larger than its parent's in a well-formed file
    if (parent[i] >= i) return fail(ORBFE_ERR_INVALID, "vocabulary: node listed before its parent");
    off[parent[i] + 1]++;
  }
  for (int i = 0; i < n; i++) {
    if (off[i + 1] > 32) return fail(ORBFE_ERR_INVALID, "vocabulary: a node has more than 32 children");
    off[i + 1] += off[i];
  }
  std::vector<int32_t> cur(off.begin(), off.begin() + n);
  for (int i = 1; i < n; i++) idx[cur[parent[i]]++] = i;  // children in file order (:1386)
  // breadth-first positions: the children of a node become adjacent records, in file order
  std::vector<int32_t> order((size_t)n), pos((size_t)n);
  order[0] = 0;
  int filled = 1;
  for (int q = 0; q < filled; q++) {
    const int id = order[q];
    pos[id] = q;
    for (int c = off[id]; c < off[id + 1]; c++) order[filled++] = idx[c];
  }
  if (filled != n) return fail(ORBFE_ERR_INVALID, "vocabulary: unreachable nodes");
  std::vector<VocabNode> rec((size_t)n);
  std::vector<double> wpos((size_t)n);
  for (int q = 0; q < n; q++) {
    const int id = order[q];
    VocabNode& r = rec[q];
    memcpy(r.d, desc + (size_t)id * 32, 32);
    const int nc = off[id + 1] - off[id];
    r.firstChild = nc ? (uint32_t)pos[idx[off[id]]] : 0u;  // == q's children are consecutive from here
    r.nChild = (uint32_t)nc | (weight[id] > 0 ? 0x100u : 0u);
    r.id = (uint32_t)id;
    r.word = wordId[id];
    wpos[q] = weight[id];
  }
  HIPCHK(hipSetDevice(v->device));
  HIPCHK(hipStreamCreateWithFlags(&v->stream, hipStreamNonBlocking));
  int rc;
  if ((rc = v->nodes.alloc((size_t)n)) || (rc = v->weight.alloc((size_t)n))) return rc;
  v->d.nodes = v->nodes; v->d.weight = v->weight;
  v->d.rootChildren = (uint32_t)(off[1] - off[0]);
  HIPCHK(hipMemcpy(v->nodes, rec.data(), (size_t)n * sizeof(VocabNode), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(v->weight, wpos.data(), (size_t)n * 8, hipMemcpyHostToDevice));
  return ORBFE_OK;
}

static int vocab_finish(orbfe_vocabulary* v, const std::vector<int32_t>& parent, const std::vector<uint8_t>& desc,
                        const std::vector<double>& weight, const std::vector<int32_t>& wordId, orbfe_vocabulary** out) {
  int rc = vocab_upload(v, parent.data(), desc.data(), weight.data(), wordId.data());
  if (rc) { vocab_destroy_sync_objects(v); delete v; return rc; }
  *out = v;
  return ORBFE_OK;
}

extern "C" int orbfe_vocabulary_load_text(const char* path, int device, orbfe_vocabulary** out) {
  if (!path || !out) return fail(ORBFE_ERR_INVALID, "vocabulary_load_text: NULL argument");
  *out = nullptr;
  FILE* fp = fopen(path, "rb");
  if (!fp) return fail(ORBFE_ERR_INVALID, std::string("vocabulary_load_text: cannot open ") + path);
  std::string txt;  // ORBvoc.txt is 145 MB: one read, then pointer parsing (no stream per line)
  {
    char buf[1 << 16];
    size_t got;
    while ((got = fread(buf, 1, sizeof buf, fp)) > 0) txt.append(buf, got);
    fclose(fp);
  }
  char* p = &txt[0];
  char* const end = p + txt.size();  // (*end is the string's own NUL)
  auto line_end = [&](char* q) { while (q < end && *q != '\n') q++; return q; };
  if (p == end) return fail(ORBFE_ERR_INVALID, "vocabulary_load_text: empty file");
  int k = -1, L = -1, n1 = -1, n2 = -1;
  {
    const std::string head(p, line_end(p));
    std::stringstream ss(head);
    ss >> k >> L >> n1 >> n2;
  }
  if (k < 0 || k > 20 || L < 1 || L > 10 || n1 < 0 || n1 > 5 || n2 < 0 || n2 > 3)  // :1357-1361
    return fail(ORBFE_ERR_INVALID, "vocabulary_load_text: not a DBoW2 text vocabulary");
  std::vector<int32_t> parent(1, 0), wordId(1, -1);
  std::vector<uint8_t> desc(32, 0);
  std::vector<double> weight(1, 0.0);
  const size_t guess = txt.size() / 100 + 16;
  parent.reserve(guess); wordId.reserve(guess); weight.reserve(guess); desc.reserve(guess * 32);
  int nWords = 0;
  p = line_end(p);
  while (p < end) {
    p++;  // the '\n'
    char* le = line_end(p);
    const char* q = p;
    while (q < le && (*q == ' ' || *q == '\t' || *q == '\r')) q++;
    if (q < le) {  // see orbfe.h: empty lines are ignored
      // A node is ONE line (the reference parses each through its own getline + stringstream, :1374-1417): the line is
      // NUL-terminated in place so that strtol / strtod -- which skip '\n' as white space -- cannot run on into the next
      // node's tokens; the fields a short line lacks read as 0, like the reference's failed `>>` extractions
      *le = 0;
      char* r;
      const long pid = strtol(q, &r, 10);
      const long leaf = strtol(r, &r, 10);
      uint8_t d[32];
      for (int i = 0; i < 32; i++) d[i] = (uint8_t)strtol(r, &r, 10);
      const double w = strtod(r, &r);
      parent.push_back((int32_t)pid);
      desc.insert(desc.end(), d, d + 32);
      weight.push_back(w);
      wordId.push_back(leaf > 0 ? nWords++ : -1);
    }
    p = le;
  }
  orbfe_vocabulary* v = new (std::nothrow) orbfe_vocabulary();
  if (!v) return fail(ORBFE_ERR_NOMEM, "out of memory");
  v->device = device; v->k = k; v->L = L; v->scoring = n1; v->weighting = n2;
  v->nNodes = (int)parent.size();
  v->nWords = nWords;
  return vocab_finish(v, parent, desc, weight, wordId, out);
}

// The same tree from arrays (what the lines of the text file hold, node i+1 = entry i): a vocabulary built or
// converted by the caller, or a synthetic one of ORBvoc's size without a 145 MB text detour.
extern "C" int orbfe_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t* parent,
                                       const uint8_t* is_leaf, const uint8_t* descriptors, const double* weight,
                                       int device, orbfe_vocabulary** out) {
  if (!out) return fail(ORBFE_ERR_INVALID, "vocabulary_create: NULL argument");
  *out = nullptr;
  if (n_nodes < 0 || (n_nodes > 0 && (!parent || !is_leaf || !descriptors || !weight)))
    return fail(ORBFE_ERR_INVALID, "vocabulary_create: NULL argument");
  if (k < 0 || k > 20 || L < 1 || L > 10 || scoring < 0 || scoring > 5 || weighting < 0 || weighting > 3)
    return fail(ORBFE_ERR_INVALID, "vocabulary_create: header values out of range (:1357-1361)");
  const size_t n = (size_t)n_nodes + 1;
  std::vector<int32_t> par(n, 0), wordId(n, -1);
  std::vector<uint8_t> desc(n * 32, 0);
  std::vector<double> wt(n, 0.0);
  int nWords = 0;
  for (int i = 0; i < n_nodes; i++) {
    par[i + 1] = parent[i];
    wt[i + 1] = weight[i];
    wordId[i + 1] = is_leaf[i] ? nWords++ : -1;
  }
  if (n_nodes) memcpy(desc.data() + 32, descriptors, (size_t)n_nodes * 32);
  orbfe_vocabulary* v = new (std::nothrow) orbfe_vocabulary();
  if (!v) return fail(ORBFE_ERR_NOMEM, "out of memory");
  v->device = device; v->k = k; v->L = L; v->scoring = scoring; v->weighting = weighting;
  v->nNodes = (int)n;
  v->nWords = nWords;
  return vocab_finish(v, par, desc, wt, wordId, out);
}

extern "C" void orbfe_vocabulary_destroy(orbfe_vocabulary* v) {
  if (!v) return;
  (void)hipSetDevice(v->device);
  if (v->stream) (void)hipStreamSynchronize(v->stream);
  vocab_destroy_sync_objects(v);
  delete v;
}

extern "C" int orbfe_vocabulary_info(const orbfe_vocabulary* v, int* k, int* L, int* n_nodes, int* n_words) {
  if (!v) return fail(ORBFE_ERR_INVALID, "NULL vocabulary");
  if (k) *k = v->k;
  if (L) *L = v->L;
  if (n_nodes) *n_nodes = v->nNodes;
  if (n_words) *n_words = v->nWords;
  return ORBFE_OK;
}

extern "C" int orbfe_vocabulary_transform(orbfe_vocabulary* v, const uint8_t* descriptors, int n, int levelsup,
                                          uint32_t* word_id, double* weight, uint32_t* node_id) {
  if (!v || n < 0 || (n > 0 && (!descriptors || !word_id || !weight || !node_id)))
    return fail(ORBFE_ERR_INVALID, "vocabulary_transform: bad argument");
  if (n == 0) return 0;
  const size_t N = (size_t)n;
  uint8_t* ddesc;
  uint32_t *dword, *dnode;
  double* dweight;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TRY(up(a, &ddesc, descriptors, N * 32));
    open_span(a);  // the three outputs adjacent: one copy back
    dweight = carve<double>(a, N);
    dword = carve<uint32_t>(a, N);
    dnode = carve<uint32_t>(a, N);
    return close_span(a);
  };
  HIPCHK(arena_stage(v->device, &ar, stage));
  HIPCHK(flush(ar));
  launch_vocab_transform(ar->stream, v->d, ddesc, nullptr, n, n, 1, 1, v->L - levelsup, dword, dweight, dnode, nullptr);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  memcpy(word_id, mirror_of(ar, dword), N * 4);
  memcpy(weight, mirror_of(ar, dweight), N * 8);
  memcpy(node_id, mirror_of(ar, dnode), N * 4);
  int used = 0;
  for (int i = 0; i < n; i++) used += weight[i] > 0;
  return used;
}

// The BowVector of transform(features, BowVector&, FeatureVector&, levelsup) (:1127-1194) for L1_NORM / TF_IDF:
// addWeight(word, weight) in feature order for the features with weight > 0 (BowVector.cpp:34-46), then
// normalize(L1): the sum of fabs over the map in ascending word order, and one division per entry (:62-84).
extern "C" int orbfe_vocabulary_transform_bow(orbfe_vocabulary* v, const uint8_t* descriptors, int n, int levelsup,
                                              uint32_t* word_ids, double* values, int capacity, int* n_words) {
  if (!v || n < 0 || capacity < 0 || !n_words || (n > 0 && !descriptors) || (capacity > 0 && (!word_ids || !values)))
    return fail(ORBFE_ERR_INVALID, "vocabulary_transform_bow: bad argument");
  *n_words = 0;
  if (v->scoring != 0 || v->weighting != 0)
    return fail(ORBFE_ERR_INVALID, "vocabulary_transform_bow: only L1_NORM / TF_IDF vocabularies (header 'k L 0 0')");
  const size_t m = (size_t)(n > 0 ? n : 1);
  std::vector<uint32_t> word(m), node(m);
  std::vector<double> weight(m);
  const int rc = orbfe_vocabulary_transform(v, descriptors, n, levelsup, word.data(), weight.data(), node.data());
  if (rc < 0) return rc;
  std::vector<uint32_t> order;
  order.reserve((size_t)rc);
  for (int i = 0; i < n; i++)
    if (weight[i] > 0) order.push_back((uint32_t)i);
  // by word, feature order kept inside a word: the order each map entry received its additions in
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return word[a] < word[b]; });
  std::vector<uint32_t> ids;
  std::vector<double> vals;
  for (size_t i = 0; i < order.size(); i++) {
    const uint32_t f = order[i];
    if (ids.empty() || ids.back() != word[f]) { ids.push_back(word[f]); vals.push_back(weight[f]); }
    else vals.back() += weight[f];
  }
  double norm = 0.0;
  for (double x : vals) norm += fabs(x);
  if (norm > 0.0)
    for (double& x : vals) x /= norm;
  *n_words = (int)ids.size();
  if (ids.size() > (size_t)capacity)
    return fail(ORBFE_ERR_CAPACITY, "vocabulary_transform_bow: more words than `capacity` (see n_words)");
  if (!ids.empty()) {
    memcpy(word_ids, ids.data(), ids.size() * 4);
    memcpy(values, vals.data(), vals.size() * 8);
  }
  return ORBFE_OK;
}

// the six workspace arrays hold wFrames frames of wCap features; a call that exceeds either gets arrays of exactly its size
static int ensure_bow_workspace(orbfe_vocabulary* v, int nFrames, int capacity) {
  if ((size_t)nFrames <= v->wFrames && capacity <= v->wCap) return ORBFE_OK;
  HIPCHK(hipStreamSynchronize(v->stream));
  v->wFrames = 0; v->wCap = 0;
  const size_t F = (size_t)nFrames, c = (size_t)capacity;
  int rc;
  if ((rc = v->w_nodes.alloc(F * c)) || (rc = v->w_offsets.alloc(F * (c + 1))) || (rc = v->w_indices.alloc(F * c)) ||
      (rc = v->w_count.alloc(F)) || (rc = v->w_bin.alloc(F * c)) || (rc = v->w_keys.alloc(F * c)))
    return rc;
  v->wFrames = F;
  v->wCap = capacity;
  return ORBFE_OK;
}

static int next_pow2(int x) { int p = 1; while (p < x) p <<= 1; return p; }

// DBoW2::FeatureVector of every frame of a device-resident batch (Frame::ComputeBoW, src/Frame.cc:433-440)
extern "C" int orbfe_vocabulary_featvec_batch_device(orbfe_vocabulary* v, const uint8_t* d_descriptors,
                                                     const int32_t* d_n, int n_frames, int capacity, int levelsup,
                                                     uint32_t* d_fv_nodes, int32_t* d_fv_offsets,
                                                     uint32_t* d_fv_indices, int32_t* d_fv_count, uint32_t* d_word,
                                                     double* d_weight) {
  if (!v || n_frames < 0 || capacity <= 0 || !d_descriptors || !d_n || !d_fv_nodes || !d_fv_offsets ||
      !d_fv_indices || !d_fv_count || ((d_word == nullptr) != (d_weight == nullptr)))
    return fail(ORBFE_ERR_INVALID, "vocabulary_featvec_batch_device: bad argument");
  if (n_frames == 0) return ORBFE_OK;
  const int sortN = next_pow2(capacity);
  if ((size_t)sortN * 8 > 96 * 1024) return fail(ORBFE_ERR_INVALID, "vocabulary_featvec_batch_device: capacity > 8192");
  FeatVecBatch b = {};
  b.desc = d_descriptors; b.n = d_n; b.capacity = capacity; b.sortN = sortN;
  b.word = d_word; b.weight = d_weight;
  b.fvNodes = d_fv_nodes; b.fvOffsets = d_fv_offsets; b.fvIndices = d_fv_indices; b.fvCount = d_fv_count;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {  // the key scratch between the two kernels
    b.keys = carve<unsigned long long>(a, (size_t)n_frames * capacity);
    return hipSuccess;
  };
  HIPCHK(arena_stage(v->device, &ar, stage));
  launch_vocab_featvec(ar->stream, v->d, b, n_frames, v->L - levelsup);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(ar->stream));
  return ORBFE_OK;
}

// Tracking::TrackReferenceKeyFrame-style matching over a device-resident batch: for t = 1..n-1,
// ComputeBoW of both frames then SearchByBoW(KF = frame t-1 with a MapPoint on every feature,
// F = frame t)  (src/Tracking.cc:836-843, src/ORBmatcher.cc:185-325).
// e != NULL: enqueue on the extractor's stream, ordered behind every sub-batch of its last extract call, and
// return without waiting (orbfe_extractor_synchronize() to wait); e == NULL: the vocabulary's own stream, waits.
// step: frame t of the call is frame slot t*step of the arrays (2 = the left frames of an L,R-interleaved stereo batch)
static int bow_match_consecutive(orbfe_vocabulary* v, orbfe_extractor* e, int n_frames,
                                 const orbfe_keypoint* d_keypoints, const uint8_t* d_descriptors,
                                 const int32_t* d_n, int capacity, int levelsup, float nnratio,
                                 int check_orientation, int32_t* d_match, int32_t* d_nmatches, int step = 1) {
  if (!v || n_frames < 0 || capacity <= 0 || capacity > 65535 || !d_keypoints || !d_descriptors || !d_n || !d_match ||
      !d_nmatches)
    return fail(ORBFE_ERR_INVALID, "bow_match_consecutive_batch_device: bad argument");
  if (n_frames < 2) return ORBFE_OK;
  const int sortN = next_pow2(capacity);
  if ((size_t)sortN * 8 > 64 * 1024) return fail(ORBFE_ERR_INVALID, "bow_match_consecutive_batch_device: capacity > 8192");
  HIPCHK(hipSetDevice(v->device));
  int rc;
  if ((size_t)n_frames > v->wFrames || capacity > v->wCap || (v->lastMulti && v->lastMulti != e)) {
    // the workspace may still be in use on the streams of the previous call
    if (v->lastStream) HIPCHK(hipStreamSynchronize(v->lastStream));
    if (v->lastMulti && (rc = orbfe_extractor_synchronize(v->lastMulti))) return rc;
    v->lastMulti = nullptr;
  }
  rc = ensure_bow_workspace(v, n_frames, capacity);
  if (rc) return rc;
  FeatVecBatch fb = {};
  fb.desc = d_descriptors; fb.n = d_n; fb.capacity = capacity; fb.sortN = sortN; fb.frameStep = step;
  fb.fvNodes = v->w_nodes; fb.fvOffsets = v->w_offsets; fb.fvIndices = v->w_indices; fb.fvCount = v->w_count;
  fb.keys = v->w_keys;
  BowBatch bb = {};
  bb.kp = reinterpret_cast<const float*>(d_keypoints); bb.desc = d_descriptors; bb.capacity = capacity; bb.frameStep = step;
  bb.fvNodes = v->w_nodes; bb.fvOffsets = v->w_offsets; bb.fvIndices = v->w_indices; bb.fvCount = v->w_count;
  bb.nnratio = nnratio; bb.match = d_match; bb.bin = v->w_bin;
  const size_t c = (size_t)capacity;
  // nodes at level L - levelsup of a k-ary tree: at most k^level (FeatureVector entries per frame)
  int maxNodes = 1;
  for (int l = 0; l < v->L - levelsup && maxNodes < capacity; l++) maxNodes = maxNodes > capacity / (v->k > 1 ? v->k : 1) ? capacity : maxNodes * v->k;
  auto featvec_range = [&](hipStream_t st, int f0, int n) {
    FeatVecBatch r = fb;
    r.desc += (size_t)f0 * step * c * 32; r.n += (size_t)f0 * step;
    r.fvNodes += (size_t)f0 * c; r.fvOffsets += (size_t)f0 * (c + 1); r.fvIndices += (size_t)f0 * c; r.fvCount += f0;
    r.keys += (size_t)f0 * c;
    launch_vocab_featvec(st, v->d, r, n, v->L - levelsup);
  };
  auto search_range = [&](hipStream_t st, int p0, int np) -> int {
    if (np <= 0) return ORBFE_OK;
    HIPCHK(hipMemsetAsync(d_match + (size_t)p0 * c, 0xff, (size_t)np * c * 4, st));
    HIPCHK(hipMemsetAsync(v->w_bin + (size_t)p0 * c, 0, (size_t)np * c, st));
    BowBatch r = bb;
    r.kp += (size_t)p0 * step * c * 7; r.desc += (size_t)p0 * step * c * 32;
    r.fvNodes += (size_t)p0 * c; r.fvOffsets += (size_t)p0 * (c + 1); r.fvIndices += (size_t)p0 * c; r.fvCount += p0;
    r.match += (size_t)p0 * c; r.bin += (size_t)p0 * c;
    launch_search_by_bow_batch(st, r, np, check_orientation, d_nmatches + p0, maxNodes);
    return ORBFE_OK;
  };
  if (e) {
    SubSplit ex;
    hipStream_t streams[32];  // orbfe_extractor::kMaxStreams
    hipEvent_t chunkDone[32];
    if ((rc = orbfe_extractor_split_(e, &ex, streams, chunkDone))) return rc;
    if (!ex.lanes && ex.S > 1 && ex.frames == n_frames * step && ex.per % step == 0 && ex.per / step >= 2) {
      SubSplit sp = ex;  // in frames of THIS call
      sp.frames = n_frames;
      sp.per = ex.per / step;
      // Per sub-batch, on the sub-batch's own stream right behind its extraction (no join of the streams): the
      // FeatureVectors of its frames, then its consecutive pairs.  The pair that straddles two sub-batches
      // (last frame of i-1, first frame of i) runs on stream i behind an event of stream i-1's FeatureVectors, and
      // stream i-1 is made to wait for it before anything enqueued later (the next extract call) overwrites that frame.
      if (v->lastStream) { HIPCHK(hipStreamSynchronize(v->lastStream)); v->lastStream = nullptr; }
      v->lastMulti = e;
      for (int i = 0; i < 32; i++)
        if (!v->evFv[i]) {
          HIPCHK(hipEventCreateWithFlags(&v->evFv[i], hipEventDisableTiming));
          HIPCHK(hipEventCreateWithFlags(&v->evBoundary[i], hipEventDisableTiming));
        }
      int f0, n;
      for (int i = 0; sp.range(i, &f0, &n); i++) {
        orbfe_extractor_stage_mark_(e, ORBFE_STAGE_MATCH, i, 0, streams[i], n);
        featvec_range(streams[i], f0, n);
        HIPCHK(hipEventRecord(v->evFv[i], streams[i]));
      }
      for (int i = 0; sp.range(i, &f0, &n); i++) {
        if (i > 0) {
          // the straddling pair first, on its own: the earlier stream is released as soon as this one launch is done
          // instead of after the whole sub-batch's pairs
          HIPCHK(hipStreamWaitEvent(streams[i], v->evFv[i - 1], 0));
          if ((rc = search_range(streams[i], f0 - 1, 1))) return rc;
          HIPCHK(hipEventRecord(v->evBoundary[i], streams[i]));
          HIPCHK(hipStreamWaitEvent(streams[i - 1], v->evBoundary[i], 0));
        }
        if ((rc = search_range(streams[i], f0, n - 1))) return rc;
        orbfe_extractor_stage_mark_(e, ORBFE_STAGE_MATCH, i, 1, streams[i], n);
        if (i > 0) HIPCHK(hipEventRecord(chunkDone[i], streams[i]));  // "sub-batch i done" now includes its matcher
      }
      HIPCHK(hipGetLastError());
      return ORBFE_OK;
    }
  }
  if (v->lastMulti) {  // back to one stream after a per-sub-batch call
    if ((rc = orbfe_extractor_synchronize(v->lastMulti))) return rc;
    v->lastMulti = nullptr;
  }
  hipStream_t s = v->stream;
  if (e) {
    if ((rc = orbfe_extractor_consumer_begin_(e, &s))) return rc;
    if (v->lastStream && v->lastStream != s) HIPCHK(hipStreamSynchronize(v->lastStream));
  } else if (v->lastStream && v->lastStream != s) {
    HIPCHK(hipStreamSynchronize(v->lastStream));
  }
  v->lastStream = s;
  featvec_range(s, 0, n_frames);
  if ((rc = search_range(s, 0, n_frames - 1))) return rc;
  HIPCHK(hipGetLastError());
  if (e) return orbfe_extractor_consumer_end_(e);
  HIPCHK(hipStreamSynchronize(s));
  return ORBFE_OK;
}

extern "C" int orbfe_bow_match_consecutive_batch_device(orbfe_vocabulary* v, int n_frames,
                                                        const orbfe_keypoint* d_keypoints,
                                                        const uint8_t* d_descriptors, const int32_t* d_n,
                                                        int capacity, int levelsup, float nnratio,
                                                        int check_orientation, int32_t* d_match,
                                                        int32_t* d_nmatches) {
  return bow_match_consecutive(v, nullptr, n_frames, d_keypoints, d_descriptors, d_n, capacity, levelsup, nnratio,
                               check_orientation, d_match, d_nmatches);
}

extern "C" int orbfe_bow_match_consecutive_batch_device_async(orbfe_vocabulary* v, orbfe_extractor* e, int n_frames,
                                                              const orbfe_keypoint* d_keypoints,
                                                              const uint8_t* d_descriptors, const int32_t* d_n,
                                                              int capacity, int levelsup, float nnratio,
                                                              int check_orientation, int32_t* d_match,
                                                              int32_t* d_nmatches) {
  if (!e) return fail(ORBFE_ERR_INVALID, "bow_match_consecutive_batch_device_async: NULL extractor");
  return bow_match_consecutive(v, e, n_frames, d_keypoints, d_descriptors, d_n, capacity, levelsup, nnratio,
                               check_orientation, d_match, d_nmatches);
}

// The same over the LEFT frames of an (L0, R0, L1, R1, ...) stereo batch: Frame::ComputeBoW and SearchByBoW work on a
// stereo Frame's left keypoints (mvKeys / mDescriptors, src/Frame.cc:61-117); pair t-1 against pair t for t = 1..n_pairs-1.
extern "C" int orbfe_bow_match_consecutive_stereo_batch_device_async(orbfe_vocabulary* v, orbfe_extractor* e, int n_pairs,
                                                                     const orbfe_keypoint* d_keypoints,
                                                                     const uint8_t* d_descriptors, const int32_t* d_n,
                                                                     int capacity, int levelsup, float nnratio,
                                                                     int check_orientation, int32_t* d_match,
                                                                     int32_t* d_nmatches) {
  if (!e) return fail(ORBFE_ERR_INVALID, "bow_match_consecutive_stereo_batch_device_async: NULL extractor");
  return bow_match_consecutive(v, e, n_pairs, d_keypoints, d_descriptors, d_n, capacity, levelsup, nnratio,
                               check_orientation, d_match, d_nmatches, 2);
}
