// matcher.hip -- C-ABI entry points of the searches (include/orbfe.h, "Matcher"): the Hamming utilities, the FeatureVector
// searches (SearchByBoW, SearchForTriangulation), the stereo matcher, and the window searches (GetFeaturesInArea, the
// projection searches, Fuse, SearchBySim3) on host arrays, with the machinery of a window-search call (window_call.h).
// Stateless and re-entrant: every call runs on the calling thread's own arena and stream (arena.h); resident frames are
// frame.h / frames.hip, the searches on the resident map points mappoints_search.hip.
#include <hip/hip_runtime.h>

#include <climits>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "frame.h"
#include "host_internal.h"
#include "kernels.h"
#include "match_kernels.h"
#include "window_call.h"

using namespace orbfe;

namespace {

// merge-walk of the two ascending node-id lists (the std::map iteration + lower_bound of
// src/ORBmatcher.cc:211-300)
void shared_nodes(const orbfe_featvec* f1, const orbfe_featvec* f2, std::vector<NodePair>* out) {
  int a = 0, b = 0;
  while (a < f1->n_nodes && b < f2->n_nodes) {
    const uint32_t ia = f1->node_ids[a], ib = f2->node_ids[b];
    if (ia == ib) {
      out->push_back(NodePair{f1->offsets[a], f1->offsets[a + 1] - f1->offsets[a], f2->offsets[b],
                              f2->offsets[b + 1] - f2->offsets[b]});
      a++;
      b++;
    } else if (ia < ib) a++;
    else b++;
  }
}

}  // namespace

extern "C" int orbfe_descriptor_distance(int device, const uint8_t* a, const uint8_t* b, int n, int32_t* out) {
  if (n < 0 || (n > 0 && (!a || !b || !out))) return fail(ORBFE_ERR_INVALID, "descriptor_distance: bad argument");
  if (n == 0) return ORBFE_OK;
  Arena* ar;
  uint8_t *da, *db;
  int32_t* dout;
  auto stage = [&](Arena* s) -> hipError_t {
    TRY(up(s, &da, a, (size_t)n * 32));
    TRY(up(s, &db, b, (size_t)n * 32));
    dout = carve<int32_t>(s, n);
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_hamming_pairs(ar->stream, da, db, n, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, ar->stream));
  HIPCHK(hipStreamSynchronize(ar->stream));
  return ORBFE_OK;
}

extern "C" int orbfe_hamming_matrix(int device, const uint8_t* d1, int n1, const uint8_t* d2, int n2, int32_t* out) {
  if (n1 < 0 || n2 < 0 || ((n1 > 0 && n2 > 0) && (!d1 || !d2 || !out)))
    return fail(ORBFE_ERR_INVALID, "hamming_matrix: bad argument");
  if (n1 == 0 || n2 == 0) return ORBFE_OK;
  Arena* ar;
  uint8_t *da, *db;
  int32_t* dout;
  auto stage = [&](Arena* s) -> hipError_t {
    TRY(up(s, &da, d1, (size_t)n1 * 32));
    TRY(up(s, &db, d2, (size_t)n2 * 32));
    dout = carve<int32_t>(s, (size_t)n1 * n2);
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_hamming_matrix(ar->stream, da, n1, db, n2, dout);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(out, dout, (size_t)n1 * n2 * 4, hipMemcpyDeviceToHost, ar->stream));
  HIPCHK(hipStreamSynchronize(ar->stream));
  return ORBFE_OK;
}

// ---------------------------------------------------------------------------------------------
// The FeatureVector searches, ORBmatcher::SearchByBoW and SearchForTriangulation: ONE implementation each, of one
// operand against K others.  The entry points differ only in where an operand's arrays are -- host arrays travel with
// the call, a resident frame has them on the device -- and in K.
// ---------------------------------------------------------------------------------------------
namespace {
// One side of a search.  h*: host arrays -- what a side without a frame uploads, and what the query list and the octave
// check read; d*: what the kernels read.  Only what the search needs is set (SearchByBoW: no x / y / octave / stereo).
struct FvSide {
  int n = 0;
  const orbfe_featvec* fv = nullptr;
  const orbfe_frame* frame = nullptr;  // resident: the d* are the frame's own, frame_use() orders the call behind its upload
  const uint8_t *hdesc = nullptr, *hstereo = nullptr;
  const float *hangle = nullptr, *hx = nullptr, *hy = nullptr;
  const int32_t* hoct = nullptr;
  uint8_t *ddesc = nullptr, *dstereo = nullptr;
  float *dangle = nullptr, *dx = nullptr, *dy = nullptr;
  int32_t* doct = nullptr;
  uint32_t* dindices = nullptr;
};
FvSide side_of_frame(const orbfe_frame* f) {
  FvSide s;
  s.n = f->n; s.fv = &f->fv; s.frame = f; s.hstereo = f->hstereo.data(); s.hoct = f->hoct.data();
  s.ddesc = f->ddesc; s.dstereo = f->dstereo; s.dangle = f->dangle; s.dx = f->dx; s.dy = f->dy; s.doct = f->doct;
  s.dindices = f->dindices;
  return s;
}
// the host arrays of a side that no resident frame backs, into the arena
hipError_t side_upload(Arena* a, FvSide* s, bool withIndices) {
  const size_t n = (size_t)s->n;
  if (s->frame) return hipSuccess;
  if (s->hdesc) TRY(up(a, &s->ddesc, s->hdesc, n * 32));
  if (s->hstereo) TRY(up(a, &s->dstereo, s->hstereo, n));
  if (s->hx) TRY(up(a, &s->dx, s->hx, n));
  if (s->hy) TRY(up(a, &s->dy, s->hy, n));
  if (s->hangle) TRY(up(a, &s->dangle, s->hangle, n));
  if (s->hoct) TRY(up(a, &s->doct, s->hoct, n));
  if (withIndices && s->fv->n_nodes > 0) TRY(up(a, &s->dindices, s->fv->indices, (size_t)s->fv->offsets[s->fv->n_nodes]));
  return hipSuccess;
}

// SearchByBoW (src/ORBmatcher.cc:185-325, :327-464) of `one` against many[0 .. K): one upload, one group of launches,
// one download, one synchronisation.
//   kfkf = 0, (KF_k, F):  `one` is the frame (the `2` side), many[k] key frame k with mask masks[k]; match[k * one->n + i2]
//   kfkf = 1, (KF, KF_k): `one` is the `1` side with mask maskOne, many[k] the `2` side with masks[k]; match[k * one->n + i1]
// batch = 0 (K = 1): the single-problem kernels, and nothing runs when the two share no node.  The caller has checked the
// operands and initialised match / n_matches; an empty many[k] is skipped.
int bow_run(const char* who, int device, FvSide* one, const uint8_t* maskOne, int K, FvSide* many, const uint8_t* const* masks,
            float nnratio, int check_ori, int kfkf, int batch, int32_t* match, int32_t* n_matches) {
  UnsettledScope unsettledScope;
  const int nOut = one->n;
  std::vector<std::vector<NodePair>> pairs((size_t)K);
  int total = 0, maxCnt2 = 0;
  for (int k = 0; k < K; k++) {
    if (many[k].n == 0) continue;
    if (kfkf) shared_nodes(one->fv, many[k].fv, &pairs[k]); else shared_nodes(many[k].fv, one->fv, &pairs[k]);
    for (const NodePair& p : pairs[k]) maxCnt2 = p.cnt2 > maxCnt2 ? p.cnt2 : maxCnt2;
    if (maxCnt2 > 65535) return fail(ORBFE_ERR_INVALID, std::string(who) + ": more than 65535 features in one node");
    total += (int)pairs[k].size();
  }
  if (!batch && total == 0) return ORBFE_OK;
  // the problems as ONE launch: operands of problem k in hargs[k], its node pairs numbered from pairStart[k]
  std::vector<BowArgs> hargs;
  std::vector<int32_t> pairStart;
  BowArgs* dargs = nullptr;
  int32_t *dstart = nullptr, *dmatch = nullptr, *dcount = nullptr;
  int8_t* dbin = nullptr;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    uint8_t* dmOne = nullptr;
    TRY(side_upload(a, one, true));
    for (int k = 0; k < K; k++) TRY(side_upload(a, &many[k], true));
    if (kfkf) TRY(up(a, &dmOne, maskOne, (size_t)nOut));
    TRY(up_fill(a, &dmatch, (size_t)K * nOut, 0xff));  // match arrays and counts adjacent: one copy back
    TRY(up_fill(a, &dcount, (size_t)K, 0));
    TRY(up_fill(a, &dbin, (size_t)K * nOut, 0));
    hargs.clear();
    pairStart.clear();
    for (int k = 0, start = 0; k < K; start += (int)pairs[k].size(), k++) {
      if (pairs[k].empty()) continue;
      const FvSide *f1 = kfkf ? one : &many[k], *f2 = kfkf ? &many[k] : one;
      NodePair* dp;
      uint8_t* dmk;
      TRY(up(a, &dp, pairs[k].data(), pairs[k].size()));
      TRY(up(a, &dmk, masks[k], (size_t)many[k].n));
      BowArgs b = {};
      b.pairs = dp;
      b.desc1 = f1->ddesc; b.hasMp1 = kfkf ? dmOne : dmk; b.angle1 = f1->dangle; b.indices1 = f1->dindices;
      b.desc2 = f2->ddesc; b.hasMp2 = kfkf ? dmk : nullptr; b.angle2 = f2->dangle; b.indices2 = f2->dindices;
      b.angleStride = 1;
      b.nnratio = nnratio; b.strictLow = kfkf; b.match = dmatch + (size_t)k * nOut; b.bin = dbin + (size_t)k * nOut;
      hargs.push_back(b);
      pairStart.push_back(start);
    }
    if (batch && !hargs.empty()) {
      TRY(up(a, &dargs, hargs.data(), hargs.size()));
      TRY(up(a, &dstart, pairStart.data(), pairStart.size()));
    }
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(frame_use(ar, one->frame));
  for (int k = 0; k < K; k++) HIPCHK(frame_use(ar, many[k].frame));
  HIPCHK(flush(ar));
  if (batch) {
    launch_search_by_bow_multi(ar->stream, dargs, dstart, (int)hargs.size(), total, maxCnt2);
    launch_rot_prune_batch(ar->stream, dmatch, dbin, nOut, K, check_ori, dcount);  // all K histograms in one launch
  } else {
    launch_search_by_bow(ar->stream, hargs[0], total, maxCnt2);
    launch_rot_prune(ar->stream, dmatch, dbin, nOut, check_ori, dcount);
  }
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, dmatch, dcount + K));
  HIPCHK(hipStreamSynchronize(ar->stream));
  frames_settle();
  std::memcpy(match, mirror_of(ar, dmatch), (size_t)K * nOut * 4);
  std::memcpy(n_matches, mirror_of(ar, dcount), (size_t)K * 4);
  return ORBFE_OK;
}

// SearchForTriangulation (src/ORBmatcher.cc:657-822) of s1 against the neighbours many[0 .. K) (LocalMapping::
// CreateNewMapPoints, src/LocalMapping.cc:256-315: the same mpCurrentKeyFrame, a new F12 per neighbour), in one round
// trip as bow_run.  F12: [K * 9]; ex, ey: [K]; match12[k * s1->n + i1].  batch = 0 (K = 1): the single-array prune, and
// nothing runs without a query.
int tri_run(const char* who, int device, FvSide* s1, const uint8_t* has_mp1, int K, FvSide* many, const uint8_t* const* has_mp2,
            const float* F12, const float* ex, const float* ey, const float* scale_factors2, const float* level_sigma2_2,
            int n_levels2, int only_stereo, int check_ori, int batch, int32_t* match12, int32_t* n_matches) {
  UnsettledScope unsettledScope;
  const int n1 = s1->n;
  // host: the shared nodes and the query list of every neighbour (:787-811)
  std::vector<std::vector<TriQuery>> queries((size_t)K);
  std::vector<NodePair> pairs;
  size_t nQueries = 0;
  for (int k = 0; k < K; k++) {
    const FvSide& s2 = many[k];
    for (int i = 0; i < s2.n; i++)
      if (s2.hoct[i] < 0 || s2.hoct[i] >= n_levels2) return fail(ORBFE_ERR_INVALID, std::string(who) + ": octave out of range");
    pairs.clear();
    if (s2.n > 0) shared_nodes(s1->fv, s2.fv, &pairs);
    for (const NodePair& p : pairs) {
      if (p.cnt2 > 65535) return fail(ORBFE_ERR_INVALID, std::string(who) + ": more than 65535 features in one node");
      for (int i = 0; i < p.cnt1; i++) {
        const uint32_t idx1 = s1->fv->indices[p.off1 + i];
        if (has_mp1[idx1]) continue;                       // :800-803
        if (only_stereo && !s1->hstereo[idx1]) continue;   // :807-809
        queries[k].push_back(TriQuery{idx1, p.off2, p.cnt2});
      }
    }
    nQueries += queries[k].size();
  }
  if (!batch && nQueries == 0) return ORBFE_OK;
  // the problems run as ONE launch: their argument blocks and first workgroups travel with the inputs
  std::vector<TriArgs> targs;
  std::vector<int32_t> blockStart;
  int totalBlocks = 0;
  TriArgs* dargs = nullptr;
  int32_t *dstart = nullptr, *dmatch = nullptr, *dcount = nullptr;
  int8_t* dbin = nullptr;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    float *dF, *dsf, *dsg;
    TRY(side_upload(a, s1, false));  // (the queries carry the `1` side's indices)
    for (int k = 0; k < K; k++) TRY(side_upload(a, &many[k], true));
    TRY(up(a, &dF, F12, (size_t)K * 9));
    TRY(up(a, &dsf, scale_factors2, (size_t)n_levels2));
    TRY(up(a, &dsg, level_sigma2_2, (size_t)n_levels2));
    TRY(up_fill(a, &dmatch, (size_t)K * n1, 0xff));  // match arrays and counts adjacent: one copy back
    TRY(up_fill(a, &dcount, (size_t)K, 0));
    TRY(up_fill(a, &dbin, (size_t)K * n1, 0));
    targs.clear();
    blockStart.clear();
    totalBlocks = 0;
    for (int k = 0; k < K; k++) {
      if (queries[k].empty()) continue;
      const FvSide& s2 = many[k];
      TriQuery* dq;
      uint8_t* dm2;
      TRY(up(a, &dq, queries[k].data(), queries[k].size()));
      TRY(up(a, &dm2, has_mp2[k], (size_t)s2.n));
      TriArgs t = {};
      t.queries = dq; t.nQueries = (int)queries[k].size();
      t.desc1 = s1->ddesc; t.x1 = s1->dx; t.y1 = s1->dy; t.angle1 = s1->dangle; t.stereo1 = s1->dstereo;
      t.desc2 = s2.ddesc; t.hasMp2 = dm2; t.x2 = s2.dx; t.y2 = s2.dy; t.angle2 = s2.dangle; t.octave2 = s2.doct;
      t.stereo2 = s2.dstereo; t.indices2 = s2.dindices;
      t.F12 = dF + (size_t)k * 9; t.ex = ex[k]; t.ey = ey[k]; t.scaleFactors2 = dsf; t.levelSigma2_2 = dsg;
      t.onlyStereo = only_stereo; t.match = dmatch + (size_t)k * n1; t.bin = dbin + (size_t)k * n1;
      targs.push_back(t);
      blockStart.push_back(totalBlocks);
      totalBlocks += (t.nQueries + 3) / 4;
    }
    if (batch && !targs.empty()) {
      TRY(up(a, &dargs, targs.data(), targs.size()));
      TRY(up(a, &dstart, blockStart.data(), blockStart.size()));
    }
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(frame_use(ar, s1->frame));
  for (int k = 0; k < K; k++) HIPCHK(frame_use(ar, many[k].frame));
  HIPCHK(flush(ar));
  if (targs.size() == 1) launch_search_triangulation(ar->stream, targs[0]);
  else if (!targs.empty()) launch_search_triangulation_multi(ar->stream, dargs, dstart, (int)targs.size(), totalBlocks);
  if (batch) launch_rot_prune_batch(ar->stream, dmatch, dbin, n1, K, check_ori, dcount);  // all K histograms in one launch
  else launch_rot_prune(ar->stream, dmatch, dbin, n1, check_ori, dcount);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, dmatch, dcount + K));
  HIPCHK(hipStreamSynchronize(ar->stream));
  frames_settle();
  std::memcpy(match12, mirror_of(ar, dmatch), (size_t)K * n1 * 4);
  std::memcpy(n_matches, mirror_of(ar, dcount), (size_t)K * 4);
  return ORBFE_OK;
}

// the single forms in the reference's operand order.  (KF, F): the frame is bow_run's `one`, the key frame its only other
int bow_one(const char* who, int device, FvSide* s1, const uint8_t* has_mp1, FvSide* s2, const uint8_t* has_mp2,
            float nnratio, int check_ori, int kfkf, int32_t* match) {
  int32_t count = 0;
  const int rc = kfkf ? bow_run(who, device, s1, has_mp1, 1, s2, &has_mp2, nnratio, check_ori, 1, 0, match, &count)
                      : bow_run(who, device, s2, nullptr, 1, s1, &has_mp1, nnratio, check_ori, 0, 0, match, &count);
  return rc ? rc : count;
}

int bow_host(int device, const uint8_t* desc1, const uint8_t* has_mp1, const float* angle1, int n1, const orbfe_featvec* fv1,
             const uint8_t* desc2, const uint8_t* has_mp2, const float* angle2, int n2, const orbfe_featvec* fv2,
             float nnratio, int check_ori, int kfkf, int32_t* match) {
  if (n1 < 0 || n2 < 0 || !match) return fail(ORBFE_ERR_INVALID, "search_by_bow: bad argument");
  const int nOut = kfkf ? n1 : n2;
  for (int i = 0; i < nOut; i++) match[i] = -1;
  if (n1 == 0 || n2 == 0) return 0;
  if (!desc1 || !has_mp1 || !angle1 || !desc2 || !angle2 || (kfkf && !has_mp2))
    return fail(ORBFE_ERR_INVALID, "search_by_bow: NULL input");
  if (!featvec_ok(fv1, n1) || !featvec_ok(fv2, n2)) return fail(ORBFE_ERR_INVALID, "search_by_bow: malformed FeatureVector");
  FvSide s1, s2;
  s1.n = n1; s1.fv = fv1; s1.hdesc = desc1; s1.hangle = angle1;
  s2.n = n2; s2.fv = fv2; s2.hdesc = desc2; s2.hangle = angle2;
  return bow_one("search_by_bow", device, &s1, has_mp1, &s2, has_mp2, nnratio, check_ori, kfkf, match);
}

// on resident frames: per call only the shared-node list, the map-point masks and the result arrays travel
int bow_resident(const orbfe_frame* k1, const uint8_t* has_mp1, const orbfe_frame* k2, const uint8_t* has_mp2,
                 float nnratio, int check_ori, int kfkf, int32_t* match) {
  if (!k1 || !k2 || !match) return fail(ORBFE_ERR_INVALID, "search_by_bow_resident: NULL argument");
  if (k1->device != k2->device) return fail(ORBFE_ERR_INVALID, "search_by_bow_resident: frames on different devices");
  const int n1 = k1->n, n2 = k2->n, nOut = kfkf ? n1 : n2;
  for (int i = 0; i < nOut; i++) match[i] = -1;
  if (n1 == 0 || n2 == 0) return 0;
  if (!k1->haveFv || !k2->haveFv || k1->hangle.empty() || k2->hangle.empty() || !has_mp1 || (kfkf && !has_mp2))
    return fail(ORBFE_ERR_INVALID, "search_by_bow_resident: the frames were uploaded without FeatureVector / angles, or a mask is NULL");
  FvSide s1 = side_of_frame(k1), s2 = side_of_frame(k2);
  return bow_one("search_by_bow_resident", k1->device, &s1, has_mp1, &s2, has_mp2, nnratio, check_ori, kfkf, match);
}

// ONE frame / key frame against K candidate key frames in one call: Tracking::Relocalization runs
// SearchByBoW(pKF_k, mCurrentFrame, ...) over every candidate (src/Tracking.cc:1478-1498), LoopClosing::ComputeSim3
// SearchByBoW(mpCurrentKF, pKF_k, ...) (src/LoopClosing.cc:294-321).  A single resident call is a round trip of ~0.16 ms
// whatever it computes; here the K problems share one.
int bow_multi(const orbfe_frame* one, const uint8_t* has_mp_one, int K, const orbfe_frame* const* many,
              const uint8_t* const* has_mp_k, float nnratio, int check_ori, int kfkf, int32_t* match, int32_t* n_matches) {
  if (!one || K < 0 || (K > 0 && (!many || !has_mp_k || !match || !n_matches)))
    return fail(ORBFE_ERR_INVALID, "search_by_bow_multi: bad argument");
  for (size_t i = 0; i < (size_t)K * one->n; i++) match[i] = -1;
  for (int k = 0; k < K; k++) n_matches[k] = 0;
  if (K == 0 || one->n == 0) return ORBFE_OK;
  if (!one->haveFv || one->hangle.empty() || (kfkf && !has_mp_one))
    return fail(ORBFE_ERR_INVALID, "search_by_bow_multi: frame uploaded without FeatureVector / angles, or NULL mask");
  std::vector<FvSide> sides((size_t)K);
  for (int k = 0; k < K; k++) {
    const orbfe_frame* c = many[k];
    if (!c || (c->n > 0 && !has_mp_k[k])) return fail(ORBFE_ERR_INVALID, "search_by_bow_multi: NULL candidate or mask");
    if (c->device != one->device) return fail(ORBFE_ERR_INVALID, "search_by_bow_multi: frames on different devices");
    if (c->n > 0 && (!c->haveFv || c->hangle.empty()))
      return fail(ORBFE_ERR_INVALID, "search_by_bow_multi: candidate uploaded without FeatureVector / angles");
    sides[(size_t)k] = side_of_frame(c);
  }
  FvSide s = side_of_frame(one);
  return bow_run("search_by_bow_multi", one->device, &s, has_mp_one, K, sides.data(), has_mp_k, nnratio, check_ori, kfkf, 1,
                 match, n_matches);
}
}  // namespace

extern "C" int orbfe_search_by_bow(int device, const uint8_t* desc1, const uint8_t* has_mp1, const float* angle1,
                                   int n1, const orbfe_featvec* fv1, const uint8_t* desc2, const float* angle2,
                                   int n2, const orbfe_featvec* fv2, float nnratio, int check_orientation,
                                   int32_t* match_f) {
  return bow_host(device, desc1, has_mp1, angle1, n1, fv1, desc2, nullptr, angle2, n2, fv2, nnratio, check_orientation, 0,
                  match_f);
}
extern "C" int orbfe_search_by_bow_kf(int device, const uint8_t* desc1, const uint8_t* has_mp1, const float* angle1,
                                      int n1, const orbfe_featvec* fv1, const uint8_t* desc2,
                                      const uint8_t* has_mp2, const float* angle2, int n2,
                                      const orbfe_featvec* fv2, float nnratio, int check_orientation,
                                      int32_t* match12) {
  return bow_host(device, desc1, has_mp1, angle1, n1, fv1, desc2, has_mp2, angle2, n2, fv2, nnratio, check_orientation, 1,
                  match12);
}
extern "C" int orbfe_search_by_bow_resident(const orbfe_frame* kf, const uint8_t* has_mp_kf, const orbfe_frame* f,
                                            float nnratio, int check_orientation, int32_t* match_f) {
  return bow_resident(kf, has_mp_kf, f, nullptr, nnratio, check_orientation, 0, match_f);
}
extern "C" int orbfe_search_by_bow_kf_resident(const orbfe_frame* kf1, const uint8_t* has_mp1, const orbfe_frame* kf2,
                                               const uint8_t* has_mp2, float nnratio, int check_orientation,
                                               int32_t* match12) {
  return bow_resident(kf1, has_mp1, kf2, has_mp2, nnratio, check_orientation, 1, match12);
}
extern "C" int orbfe_search_by_bow_multi(int n_keyframes, const orbfe_frame* const* kf, const uint8_t* const* has_mp_kf,
                                         const orbfe_frame* f, float nnratio, int check_orientation, int32_t* match_f,
                                         int32_t* n_matches) {
  return bow_multi(f, nullptr, n_keyframes, kf, has_mp_kf, nnratio, check_orientation, 0, match_f, n_matches);
}
extern "C" int orbfe_search_by_bow_kf_multi(const orbfe_frame* kf1, const uint8_t* has_mp1, int n_keyframes,
                                            const orbfe_frame* const* kf2, const uint8_t* const* has_mp2, float nnratio,
                                            int check_orientation, int32_t* match12, int32_t* n_matches) {
  return bow_multi(kf1, has_mp1, n_keyframes, kf2, has_mp2, nnratio, check_orientation, 1, match12, n_matches);
}

extern "C" int orbfe_search_for_triangulation(int device, const uint8_t* desc1, const uint8_t* has_mp1,
                                              const float* x1, const float* y1, const float* angle1,
                                              const uint8_t* stereo1, int n1, const orbfe_featvec* fv1,
                                              const uint8_t* desc2, const uint8_t* has_mp2, const float* x2,
                                              const float* y2, const float* angle2, const int32_t* octave2,
                                              const uint8_t* stereo2, int n2, const orbfe_featvec* fv2,
                                              const float* F12, float ex, float ey, const float* scale_factors2,
                                              const float* level_sigma2_2, int n_levels2, int only_stereo,
                                              int check_orientation, int32_t* match12) {
  if (n1 < 0 || n2 < 0 || !match12) return fail(ORBFE_ERR_INVALID, "search_for_triangulation: bad argument");
  for (int i = 0; i < n1; i++) match12[i] = -1;
  if (n1 == 0 || n2 == 0) return 0;
  if (!desc1 || !has_mp1 || !x1 || !y1 || !angle1 || !stereo1 || !desc2 || !has_mp2 || !x2 || !y2 || !angle2 ||
      !octave2 || !stereo2 || !F12 || !scale_factors2 || !level_sigma2_2 || n_levels2 <= 0 || n_levels2 > ORBFE_MAX_LEVELS)
    return fail(ORBFE_ERR_INVALID, "search_for_triangulation: NULL input");
  if (!featvec_ok(fv1, n1) || !featvec_ok(fv2, n2)) return fail(ORBFE_ERR_INVALID, "search_for_triangulation: malformed FeatureVector");
  FvSide s1, s2;
  s1.n = n1; s1.fv = fv1; s1.hdesc = desc1; s1.hstereo = stereo1; s1.hx = x1; s1.hy = y1; s1.hangle = angle1;
  s2.n = n2; s2.fv = fv2; s2.hdesc = desc2; s2.hstereo = stereo2; s2.hx = x2; s2.hy = y2; s2.hangle = angle2; s2.hoct = octave2;
  int32_t count = 0;
  const int rc = tri_run("search_for_triangulation", device, &s1, has_mp1, 1, &s2, &has_mp2, F12, &ex, &ey, scale_factors2,
                         level_sigma2_2, n_levels2, only_stereo, check_orientation, 0, match12, &count);
  return rc ? rc : count;
}

extern "C" int orbfe_search_for_triangulation_multi(const orbfe_frame* kf1, const uint8_t* has_mp1, int n_neighbours,
                                                    const orbfe_frame* const* kf2, const uint8_t* const* has_mp2,
                                                    const float* F12, const float* ex, const float* ey,
                                                    const float* scale_factors2, const float* level_sigma2_2,
                                                    int n_levels2, int only_stereo, int check_orientation,
                                                    int32_t* match12, int32_t* n_matches) {
  if (!kf1 || n_neighbours < 0 || (n_neighbours > 0 && (!kf2 || !has_mp2 || !F12 || !ex || !ey || !match12 || !n_matches)) ||
      !scale_factors2 || !level_sigma2_2 || n_levels2 <= 0 || n_levels2 > ORBFE_MAX_LEVELS)
    return fail(ORBFE_ERR_INVALID, "search_for_triangulation_multi: bad argument");
  const int n1 = kf1->n, K = n_neighbours;
  for (size_t i = 0; i < (size_t)K * n1; i++) match12[i] = -1;
  for (int k = 0; k < K; k++) n_matches[k] = 0;
  if (K == 0 || n1 == 0) return ORBFE_OK;
  if (!has_mp1 || !kf1->haveFv || kf1->hangle.empty())
    return fail(ORBFE_ERR_INVALID, "search_for_triangulation_multi: key frame uploaded without FeatureVector / angles, or NULL mask");
  std::vector<FvSide> sides((size_t)K);
  for (int k = 0; k < K; k++) {
    const orbfe_frame* k2 = kf2[k];
    if (!k2 || (!has_mp2[k] && k2->n > 0)) return fail(ORBFE_ERR_INVALID, "search_for_triangulation_multi: NULL neighbour");
    if (k2->device != kf1->device) return fail(ORBFE_ERR_INVALID, "search_for_triangulation_multi: frames on different devices");
    if (k2->n > 0 && (!k2->haveFv || k2->hangle.empty()))
      return fail(ORBFE_ERR_INVALID, "search_for_triangulation_multi: neighbour uploaded without FeatureVector / angles");
    sides[(size_t)k] = side_of_frame(k2);
  }
  FvSide s1 = side_of_frame(kf1);
  return tri_run("search_for_triangulation_multi", kf1->device, &s1, has_mp1, K, sides.data(), has_mp2, F12, ex, ey,
                 scale_factors2, level_sigma2_2, n_levels2, only_stereo, check_orientation, 1, match12, n_matches);
}

extern "C" int orbfe_compute_stereo_matches(orbfe_extractor* left, int frameL, orbfe_extractor* right, int frameR,
                                            const orbfe_keypoint* kpL, const uint8_t* descL, int N,
                                            const orbfe_keypoint* kpR, const uint8_t* descR, int Nr, float mbf,
                                            float mb, float* uRight, float* depth) {
  if (!left || !right || N < 0 || Nr < 0 || (N > 0 && (!kpL || !descL || !uRight || !depth)) ||
      (Nr > 0 && (!kpR || !descR)))
    return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: bad argument");
  for (int i = 0; i < N; i++) { uRight[i] = -1.0f; depth[i] = -1.0f; }
  if (N == 0 || Nr == 0) return 0;
  if (Nr >= (1 << 20)) return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: too many right keypoints");
  StereoArgs a = {};
  int nlL = 0, nlR = 0, devL = 0, devR = 0;
  float scL[kMaxLevels], iscL[kMaxLevels], scR[kMaxLevels], iscR[kMaxLevels];
  const float* dTabR = nullptr;
  int rc;
  if ((rc = orbfe_stereo_views_(left, frameL, &a.pyrL, scL, iscL, &nlL, &devL, &a.scaleTab))) return rc;
  if ((rc = orbfe_stereo_views_(right, frameR, &a.pyrR, scR, iscR, &nlR, &devR, &dTabR))) return rc;
  if (nlL != nlR || devL != devR) return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: extractors differ");
  for (int l = 0; l < nlL; l++)
    if (a.pyrL.lv[l].w != a.pyrR.lv[l].w || a.pyrL.lv[l].h != a.pyrR.lv[l].h)
      return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: left/right pyramids differ in size");
  // host operands are checked here (the reference indexes mvInvScaleFactor / mvImagePyramid / vRowIndices with them
  // unchecked, src/Frame.cc:537-538,560,600-610); the device-operand form cannot look and answers "no stereo" instead
  const float W0 = (float)a.pyrL.lv[0].w, H0 = (float)a.pyrL.lv[0].h;
  for (int side = 0; side < 2; side++) {
    const orbfe_keypoint* kp = side ? kpR : kpL;
    for (int i = 0, n = side ? Nr : N; i < n; i++) {
      if (kp[i].octave < 0 || kp[i].octave >= nlL) return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: octave out of range");
      if (!(kp[i].x >= 0.f && kp[i].x < W0 && kp[i].y >= 0.f && kp[i].y < H0))  // (false for NaN too)
        return fail(ORBFE_ERR_INVALID, "compute_stereo_matches: keypoint outside the image (or not finite)");
    }
  }
  Arena* ar;
  const int rows = a.pyrL.lv[0].h;
  a.N = N; a.Nr = Nr;
  a.frameL = frameL; a.frameR = frameR;
  a.mbf = mbf;
  a.maxD = mbf / mb;  // minZ = mb, maxD = mbf/minZ (:542-544)
  int32_t* dcount = nullptr;
  auto stage = [&](Arena* s) -> hipError_t {
    float *dkl, *dkr;
    uint8_t *ddl, *ddr;
    TRY(up(s, &dkl, reinterpret_cast<const float*>(kpL), (size_t)N * 7));
    TRY(up(s, &dkr, reinterpret_cast<const float*>(kpR), (size_t)Nr * 7));
    TRY(up(s, &ddl, descL, (size_t)N * 32));
    TRY(up(s, &ddr, descR, (size_t)Nr * 32));
    a.kpL = dkl; a.descL = ddl; a.kpR = dkr; a.descR = ddr;
    a.uRight = carve<float>(s, N);
    a.depth = carve<float>(s, N);
    dcount = carve<int32_t>(s, 1);  // (right behind the two outputs: one copy brings all three back)
    a.sad = carve<int32_t>(s, N);
    if (rows + 1 <= 8192) {  // row index of the right keypoints (k_stereo_bucket)
      a.rowStart = carve<int32_t>(s, (size_t)rows + 1);
      a.sortedIdx = carve<int32_t>(s, (size_t)Nr);
      a.rows = rows;
      a.bandR = (int)std::ceil(2.0f * scL[nlL - 1]) + 2;
    }
    return hipSuccess;
  };
  HIPCHK(arena_stage(devL, &ar, stage));
  HIPCHK(flush(ar));
  launch_stereo(ar->stream, a, dcount);
  HIPCHK(hipGetLastError());
  HIPCHK(down_range(ar, a.uRight, dcount + 1));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(uRight, mirror_of(ar, a.uRight), (size_t)N * 4);
  std::memcpy(depth, mirror_of(ar, a.depth), (size_t)N * 4);
  return *mirror_of(ar, dcount);
}

// ---------------------------------------------------------------------------------------------
// Frame grid, GetFeaturesInArea and the projection searches: the machinery of one window-search
// call (window_call.h).  The device gathers every window and takes the Hamming distances (k_window.hip); the claim loops
// run behind it on the device (k_window_claim), so the candidate lists never leave it.  A call's queries travel with it as
// host arrays, or a producer (window_call.h: Producer; mappoints_search.hip) writes them on the device.
// ---------------------------------------------------------------------------------------------
namespace orbfe {
bool frame_ok(const orbfe_frame_view* f) {
  if (!f || f->n < 0 || f->n > GRID_MAX_FEATURES) return false;
  if (!(f->max_x > f->min_x) || !(f->max_y > f->min_y)) return false;
  if (f->n > 0 && (!f->x || !f->y || !f->octave)) return false;
  return true;
}
}  // namespace orbfe

namespace {

// Where a job's arrays are on the device: carved from the call's arena by the three stage_* helpers below, a slice of what
// the call's producer writes, or a resident frame's own.  NULL where the job has no such array.
struct JobDev {
  bool withDesc = false, withUr = false;  // the search takes descriptor distances / runs the stereo check
  int frameOf = -1;  // the job whose uploaded frame arrays and grid this one uses (itself: it uploads and builds); -1: resident
  float *x = nullptr, *y = nullptr, *ur = nullptr, *angle = nullptr;  // frame
  int32_t *oct = nullptr, *cell = nullptr;
  uint8_t* desc = nullptr;
  uint32_t* key = nullptr;
  float *qx = nullptr, *qy = nullptr, *qr = nullptr, *qur = nullptr;  // queries: uploaded, or the producer's
  int32_t *qmin = nullptr, *qmax = nullptr;
  uint8_t *qactive = nullptr, *qdesc = nullptr;
  float *gateUr = nullptr, *invSigma2 = nullptr;  // (BEST mode behind Fuse's gate)
  uint8_t *blocked = nullptr, *blockVal = nullptr;  // CLAIM mode: inputs, scratch, the dynamic LDS the job's workgroup needs
  float* qAngle = nullptr;
  int32_t *choice = nullptr, *link = nullptr, *owner = nullptr;
  size_t claimLds = 0;
  int32_t* count = nullptr;  // the lists: a result in list mode, the claim kernel's input in CLAIM mode
  uint32_t* cand = nullptr;
  int32_t *best = nullptr, *header = nullptr, *match = nullptr;  // results of BEST / CLAIM mode
  float *prevX = nullptr, *prevY = nullptr;
};

// Region 1 of a call's arena, job j's part: everything that travels up.  Only up() between the first and the last of these,
// so that flush()'s dirty range is exactly the uploads: one host-to-device copy.
hipError_t stage_inputs(Arena* a, const WindowJob* jobs, int j, JobDev* dev) {
  const WindowJob& J = jobs[j];
  const Producer* P = J.producer;
  JobDev& D = dev[j];
  const size_t n = (size_t)J.f->n, q = (size_t)J.nq;
  D = JobDev{};
  D.withDesc = J.f->desc && (J.qdesc || P);
  D.withUr = J.f->u_right && (P ? !J.bestOut && P->with_ur(true) : J.qur != nullptr);
  if (const orbfe_frame* R = J.f->resident) {
    D.x = R->dx; D.y = R->dy; D.oct = R->doct; D.ur = J.f->u_right ? R->dur : nullptr; D.desc = D.withDesc ? R->ddesc : nullptr;
    D.angle = R->dangle; D.key = R->dkey; D.cell = R->dcell;
  } else {
    D.frameOf = j;  // several jobs on the SAME host-array frame (one frame against K candidates): one upload, one grid
    for (int k = 0; k < j && D.frameOf == j; k++)
      if (dev[k].frameOf == k && jobs[k].f == J.f && dev[k].withDesc == D.withDesc) D.frameOf = k;
    if (D.frameOf != j) {
      const JobDev& S = dev[D.frameOf];
      D.x = S.x; D.y = S.y; D.oct = S.oct; D.ur = S.ur; D.desc = S.desc;
    } else {
      TRY(up(a, &D.x, J.f->x, n)); TRY(up(a, &D.y, J.f->y, n)); TRY(up(a, &D.oct, J.f->octave, n));
      if (J.f->u_right) TRY(up(a, &D.ur, J.f->u_right, n));
      if (D.withDesc) TRY(up(a, &D.desc, J.f->desc, n * 32));
    }
  }
  if (P) {  // (the call's producer has uploaded everything: Producer::upload)
    if (J.bestOut && J.gate) D.invSigma2 = P->invSigma2;
  } else {
    TRY(up(a, &D.qx, J.qx, q)); TRY(up(a, &D.qy, J.qy, q)); TRY(up(a, &D.qr, J.qr, q));
    TRY(up(a, &D.qmin, J.qmin, q)); TRY(up(a, &D.qmax, J.qmax, q));
    if (J.qactive) TRY(up(a, &D.qactive, J.qactive, q));
    if (D.withUr) TRY(up(a, &D.qur, J.qur, q));
    if (D.withDesc) {  // the same descriptors for several jobs (Fuse: one set of map points into K key frames): one copy
      int shared = -1;
      for (int k = 0; k < j && shared < 0; k++)
        if (dev[k].withDesc && jobs[k].qdesc == J.qdesc && jobs[k].nq == J.nq) shared = k;
      if (shared >= 0) D.qdesc = dev[shared].qdesc; else TRY(up(a, &D.qdesc, J.qdesc, q * 32));
    }
    if (J.bestOut && J.gate && J.gur) TRY(up(a, &D.gateUr, J.gur, q));
    if (J.bestOut && J.gate) TRY(up(a, &D.invSigma2, J.invSigma2, (size_t)J.nLevels));
  }
  if (const ClaimSpec* C = J.claim) {
    if (C->checkOri && !J.f->resident) TRY(up(a, &D.angle, J.f->angle, n));  // (a resident frame has its angles on the device)
    if (C->blocked) TRY(up(a, &D.blocked, C->blocked, n));
    if (C->blockVal && !P) TRY(up(a, &D.blockVal, C->blockVal, q));  // (a producer writes it: Observations() > 0)
    if (C->checkOri) TRY(up(a, &D.qAngle, C->qAngle, q));
  }
  return hipSuccess;
}

// Region 2, a job's part: what comes back, fetched with the other jobs' by ONE down_range().  No kernel wants these adjacent
// (k_window_claim takes header, match and the previous positions as separate pointers) or reads past the end of one.
void stage_outputs(Arena* a, const WindowJob& J, int K, JobDev* D) {
  const size_t n = (size_t)J.f->n, q = (size_t)J.nq;
  if (J.bestOut) {
    D->best = carve<int32_t>(a, q);
  } else if (!J.claim) {
    D->count = carve<int32_t>(a, q);
    D->cand = carve<uint32_t>(a, q * (size_t)K);
  } else {
    const bool ini = J.claim->mode == CLAIM_INIT;
    D->header = carve<int32_t>(a, 4);
    D->match = carve<int32_t>(a, ini ? q : n);
    if (ini) { D->prevX = carve<float>(a, q); D->prevY = carve<float>(a, q); }
  }
}

// k_window_claim keeps its per-feature owner stamps ([2 n], CLAIM_INIT [n]) in dynamic LDS, with the features' octave bytes
// (RATIO) behind them.  A frame too large for that (~6800 features) gets the stamps in HBM; the octave bytes stay in LDS.
struct OwnerPlace { size_t ints, ldsBytes; bool inLds; };
OwnerPlace owner_place(const WindowJob& J) {
  constexpr size_t kOwnerLds = 60 * 1024;
  const size_t n = (size_t)J.f->n, ints = (J.claim->mode == CLAIM_INIT ? 1 : 2) * n, octBytes = J.claim->mode == CLAIM_RATIO ? n : 0;
  const bool inLds = ints * 4 + octBytes <= kOwnerLds;
  return OwnerPlace{ints, (inLds ? ints * 4 : 0) + octBytes, inLds};
}

// Region 3, the producer's part: the query arrays its launch writes, for all its parts -- the one carve of them
void carve_queries(Arena* a, Producer* P, const WindowJob* jobs, int nJobs) {
  const size_t n = P->total();
  bool ur = false;
  for (int j = 0; j < nJobs; j++) ur = ur || P->with_ur(jobs[j].f->u_right != nullptr);
  QueryOut& q = P->q;
  q.x = carve<float>(a, n); q.y = carve<float>(a, n); q.r = carve<float>(a, n);
  q.minLevel = carve<int32_t>(a, n); q.maxLevel = carve<int32_t>(a, n);
  q.active = carve<uint8_t>(a, n);
  if (P->with_obs()) q.obs = carve<uint8_t>(a, n);
  if (ur) q.ur = carve<float>(a, n);
  q.desc = carve<uint8_t>(a, P->desc_rows() * 32);
}

// Region 3, job j's part: what never leaves the device -- the grid of an uploaded frame, its slice of the producer's query
// arrays, the claim kernel's lists and scratch
void stage_scratch(Arena* a, const WindowJob* jobs, int j, int K, JobDev* dev) {
  const WindowJob& J = jobs[j];
  JobDev& D = dev[j];
  const size_t n = (size_t)J.f->n, q = (size_t)J.nq;
  if (J.producer) {
    const QueryOut pq = J.producer->part_queries(J.part);
    D.qx = pq.x; D.qy = pq.y; D.qr = pq.r; D.qmin = pq.minLevel; D.qmax = pq.maxLevel; D.qactive = pq.active;
    D.qdesc = D.withDesc ? pq.desc : nullptr;
    if (pq.obs) D.blockVal = pq.obs;
    if (D.withUr) D.qur = pq.ur;
    if (J.bestOut && J.gate && J.f->u_right) D.gateUr = pq.ur;
  }
  if (D.frameOf == j) { D.key = carve<uint32_t>(a, n); D.cell = carve<int32_t>(a, 3073); }
  else if (D.frameOf >= 0) { D.key = dev[D.frameOf].key; D.cell = dev[D.frameOf].cell; }
  if (J.claim) {
    // k_window_claim reads a list as pairs of 16-byte requests, eight entries at a time and never past entry K: K is a
    // multiple of 8 and carve() aligns the first list
    D.count = carve<int32_t>(a, q); D.cand = carve<uint32_t>(a, q * (size_t)K);
    D.choice = carve<int32_t>(a, q); D.link = carve<int32_t>(a, q);
    const OwnerPlace o = owner_place(J);
    if (!o.inLds) D.owner = carve<int32_t>(a, o.ints);
    D.claimLds = o.ldsBytes;
  }
}

ClaimJob claim_job(const WindowJob& J, const JobDev& D, int K) {
  const ClaimSpec& C = *J.claim;
  ClaimJob c{};
  c.count = D.count; c.cand = D.cand; c.K = K; c.nq = J.nq; c.n = J.f->n;
  c.active = D.qactive; c.blocked = D.blocked; c.blockVal = D.blockVal;
  c.octave = D.oct; c.qAngle = D.qAngle; c.fAngle = C.checkOri ? D.angle : nullptr;
  c.fx = D.x; c.fy = D.y; c.qx = D.qx; c.qy = D.qy; c.prevX = D.prevX; c.prevY = D.prevY;
  c.mode = C.mode; c.maxDist = C.maxDist; c.checkOri = C.checkOri; c.nnratio = C.nnratio;
  c.choice = D.choice; c.link = D.link; c.owner = D.owner; c.match = D.match; c.header = D.header;
  return c;
}

WindowSearchJob search_job(const WindowJob& J, const JobDev& D, int K, int blockStart) {
  GridFrame g{};
  g.x = D.x; g.y = D.y; g.octave = D.oct; g.uRight = D.ur; g.desc = D.desc; g.n = J.f->n;
  g.minX = J.f->min_x; g.minY = J.f->min_y;
  g.wInv = 64.0f / (J.f->max_x - J.f->min_x);  // src/Frame.cc:109-110 (FRAME_GRID_COLS / ROWS)
  g.hInv = 48.0f / (J.f->max_y - J.f->min_y);
  WindowQueries w{};
  w.x = D.qx; w.y = D.qy; w.r = D.qr; w.minLevel = D.qmin; w.maxLevel = D.qmax; w.active = D.qactive; w.ur = D.qur; w.desc = D.qdesc;
  w.n = J.nq; w.K = K;
  if (J.bestOut) { w.best = D.best; w.gateUr = D.gateUr; w.invSigma2 = D.invSigma2; w.gate = J.gate; w.maxDist = J.maxDist; }
  return WindowSearchJob{g, D.key, D.cell, w, D.count, D.cand, blockStart};
}

// What arena_stage() leaves of a call: every job's pointers, the kernels' argument blocks and where they and the results are
struct WindowCall {
  std::vector<JobDev> dev;
  std::vector<ClaimJob> claims;
  std::vector<WindowSearchJob> searches;
  ClaimJob* dClaims = nullptr;
  WindowSearchJob* dSearches = nullptr;  // (a single job travels as kernel arguments)
  uint8_t *outLo = nullptr, *outHi = nullptr;
  size_t claimLds = 0;
  int totalBlocks = 0;
};

// The arena of a call, in the order that keeps it at one copy each way: uploads | results | what stays on the device.  The
// argument blocks hold device addresses, known once everything is carved: they get their room behind the other uploads
// and are put() there at the end.  P: the call's producer or NULL; every pass leaves its device pointers anew.
hipError_t stage_call(Arena* a, const WindowJob* jobs, int nJobs, Producer* P, int nClaim, int K, WindowCall* c) {
  *c = WindowCall{};
  c->dev.resize((size_t)nJobs);
  if (P) {
    P->q = QueryOut{};
    TRY(P->upload(a));
  }
  for (int j = 0; j < nJobs; j++) TRY(stage_inputs(a, jobs, j, c->dev.data()));
  c->dClaims = carve<ClaimJob>(a, (size_t)nClaim);
  c->dSearches = carve<WindowSearchJob>(a, nJobs > 1 ? (size_t)nJobs : 0);
  c->outLo = carve<uint8_t>(a, 0);
  for (int j = 0; j < nJobs; j++) stage_outputs(a, jobs[j], K, &c->dev[j]);
  if (P && P->flagsOut) P->q.validCopy = carve<uint8_t>(a, P->total());
  c->outHi = carve<uint8_t>(a, 0);
  if (P) carve_queries(a, P, jobs, nJobs);
  for (int j = 0; j < nJobs; j++) stage_scratch(a, jobs, j, K, c->dev.data());
  for (int j = 0; j < nJobs; j++) {
    if (jobs[j].claim) {
      c->claims.push_back(claim_job(jobs[j], c->dev[j], K));
      if (c->dev[j].claimLds > c->claimLds) c->claimLds = c->dev[j].claimLds;
    }
    c->searches.push_back(search_job(jobs[j], c->dev[j], K, c->totalBlocks));
    c->totalBlocks += (jobs[j].nq + 3) / 4;
  }
  TRY(put(a, c->dClaims, c->claims.data(), c->claims.size()));
  if (nJobs > 1) TRY(put(a, c->dSearches, c->searches.data(), c->searches.size()));
  return hipSuccess;
}

// The call on the thread's stream: one copy up, the producer's launch, one grid build per uploaded frame, ONE window-search
// launch for all jobs, one claim launch, one copy down
hipError_t enqueue_call(Arena* ar, const WindowJob* jobs, int nJobs, Producer* P, const WindowCall& c, bool claimInit) {
  for (int j = 0; j < nJobs; j++) TRY(frame_use(ar, jobs[j].f->resident));
  TRY(flush(ar));
  if (P) TRY(P->launch(ar->stream));  // the windows of all its parts
  for (int j = 0; j < nJobs; j++)
    if (c.dev[j].frameOf == j) {
      launch_grid_build(ar->stream, c.searches[j].f, c.dev[j].key, c.dev[j].cell);
      TRY(hipGetLastError());
    }
  if (nJobs > 1) {
    launch_window_search_multi(ar->stream, c.dSearches, nJobs, c.totalBlocks);
  } else {
    const WindowSearchJob& s = c.searches[0];
    launch_window_search(ar->stream, s.f, s.sortedKey, s.cellOff, s.q, s.count, s.cand);
  }
  TRY(hipGetLastError());
  if (!c.claims.empty()) {
    launch_window_claim(ar->stream, c.dClaims, mirror_of(ar, c.dClaims), (int)c.claims.size(), c.claimLds, claimInit);
    TRY(hipGetLastError());
  }
  return down_range(ar, c.outLo, c.outHi);
}

// Behind the synchronisation: the producer's flags and every job's results out of the mirror, by mode.  Returns the longest
// list of the call; one longer than K was truncated, and a claim job that saw one has no result yet.
thread_local int t_lastClaimRounds = 0;
int collect_results(Arena* ar, const WindowJob* jobs, int nJobs, const Producer* P, const WindowCall& c, int K) {
  int mx = 0;
  if (P && P->flagsOut && P->total()) std::memcpy(P->flagsOut, mirror_of(ar, P->q.validCopy), P->total());
  for (int j = 0; j < nJobs; j++) {
    const WindowJob& J = jobs[j];
    const JobDev& D = c.dev[j];
    const size_t q = (size_t)J.nq;
    if (J.bestOut) {
      if (q) std::memcpy(J.bestOut, mirror_of(ar, D.best), q * 4);
    } else if (ClaimSpec* C = J.claim) {
      const int32_t* hd = mirror_of(ar, D.header);  // largest list length, matches, rounds
      mx = hd[0] > mx ? hd[0] : mx;
      if (hd[0] > K) continue;
      const bool ini = C->mode == CLAIM_INIT;
      const size_t nOut = ini ? q : (size_t)J.f->n;
      if (nOut) std::memcpy(C->match, mirror_of(ar, D.match), nOut * 4);
      *C->nMatches = hd[1];
      C->rounds = hd[2];
      t_lastClaimRounds = hd[2] + 1 > t_lastClaimRounds ? hd[2] + 1 : t_lastClaimRounds;
      if (ini && q) { std::memcpy(C->prevX, mirror_of(ar, D.prevX), q * 4); std::memcpy(C->prevY, mirror_of(ar, D.prevY), q * 4); }
    } else {
      const int32_t* cnt = mirror_of(ar, D.count);
      const uint32_t* cand = mirror_of(ar, D.cand);
      J.res->count.assign(cnt, cnt + q);
      J.res->cand.assign(cand, cand + q * (size_t)K);
      J.res->K = K;
      for (size_t i = 0; i < q; i++) mx = cnt[i] > mx ? cnt[i] : mx;
    }
  }
  return mx;
}

}  // namespace

namespace orbfe {

int window_search_multi(int device, WindowJob* jobs, int nJobs, int K0) {
  UnsettledScope unsettledScope;
  t_lastClaimRounds = 0;
  int nClaim = 0;
  bool claimInit = false;
  Producer* P = nJobs > 0 ? jobs[0].producer : nullptr;
  for (int j = 0; j < nJobs; j++) {
    const WindowJob& J = jobs[j];
    if (J.f->resident && J.f->resident->device != device) return fail(ORBFE_ERR_INVALID, "resident frame lives on another device");
    if (J.producer != P) return fail(ORBFE_ERR_INVALID, "the jobs of a call name one producer, or none does");
    if (P) {
      if (J.part < 0 || J.part >= P->parts() || J.nq != P->queries(J.part))
        return fail(ORBFE_ERR_INVALID, "a job behind a producer searches one of its parts, with that part's queries");
      if (const char* e = P->accepts(J.bestOut != nullptr, J.claim ? J.claim->mode : -1)) return fail(ORBFE_ERR_INVALID, e);
    }
    if (!J.claim) continue;
    if (J.nq > 0x1fffff) return fail(ORBFE_ERR_INVALID, "more than 2097151 points in one projection search");
    if (nClaim && claimInit != (J.claim->mode == CLAIM_INIT)) return fail(ORBFE_ERR_INVALID, "mixed claim forms in one call");
    claimInit = J.claim->mode == CLAIM_INIT;
    nClaim++;
  }
  WindowCall call;
  for (int K = ((K0 < 8 ? 8 : K0) + 7) & ~7;;) {  // (k_window_claim reads the lists eight entries at a time)
    Arena* ar;
    auto stage = [&](Arena* a) { return stage_call(a, jobs, nJobs, P, nClaim, K, &call); };
    HIPCHK(arena_stage(device, &ar, stage));
    HIPCHK(enqueue_call(ar, jobs, nJobs, P, call, claimInit));
    HIPCHK(hipStreamSynchronize(ar->stream));
    frames_settle();
    const int mx = collect_results(ar, jobs, nJobs, P, call, K);
    if (mx <= K) return ORBFE_OK;
    K = (mx + 7) & ~7;  // a window held more features than the list: search again with room for the largest
  }
}

int producer_run(int device, Producer& P, int n4, void* const* out4, uint8_t* flags) {
  const size_t q = P.total();
  void* d4[8] = {};
  uint8_t* dflags = nullptr;
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    P.q = QueryOut{};  // no windows: the projection alone
    TRY(P.upload(a));
    open_span(a);  // the outputs adjacent: one copy back
    for (int i = 0; i < n4; i++) d4[i] = carve<float>(a, q);
    dflags = carve<uint8_t>(a, q);
    P.project_to(d4, dflags);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  HIPCHK(P.launch(ar->stream));
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  for (int i = 0; i < n4; i++)
    if (out4[i]) std::memcpy(out4[i], mirror_of(ar, static_cast<const uint8_t*>(d4[i])), q * 4);
  if (flags) std::memcpy(flags, mirror_of(ar, dflags), q);
  return ORBFE_OK;
}

ClaimSpec last_frame_claim(const uint8_t* blocked, const uint8_t* obs_positive, const float* last_angle, int check_orientation,
                           int32_t* match_cur, int32_t* n_matches) {
  ClaimSpec C;
  C.mode = CLAIM_BEST; C.maxDist = 100 /* TH_HIGH */; C.checkOri = check_orientation ? 1 : 0;
  C.blocked = blocked;        // mvpMapPoints[i2] set with Observations() > 0 at entry (:1572-1574)
  C.blockVal = obs_positive;  // (a track producer writes it from the table's flags)
  C.qAngle = last_angle;
  C.match = match_cur; C.nMatches = n_matches;
  return C;
}
ClaimSpec keyframe_claim(const uint8_t* blocked, const float* kf_angle, int orb_dist, int check_orientation, int32_t* match_cur,
                         int32_t* n_matches) {
  ClaimSpec C;
  C.mode = CLAIM_BEST; C.maxDist = orb_dist; C.checkOri = check_orientation ? 1 : 0;
  C.blocked = blocked; C.qAngle = kf_angle;
  C.match = match_cur; C.nMatches = n_matches;
  return C;
}

int level_queries(const char* who, int n, const uint8_t* valid, const int32_t* level, const float* sf, int n_levels, float th, int lo,
                  int hi, bool no_filter, std::vector<float>* qr, std::vector<int32_t>* qmin, std::vector<int32_t>* qmax) {
  qr->resize(n); qmin->resize(n); qmax->resize(n);
  for (int i = 0; i < n; i++) {
    int lv = 0;
    if (valid[i]) {
      lv = level[i];
      if (lv < 0 || lv >= n_levels) return fail(ORBFE_ERR_INVALID, std::string(who) + ": level outside the pyramid");
    }
    (*qr)[i] = th * sf[lv];
    (*qmin)[i] = no_filter ? -1 : lv + lo;
    (*qmax)[i] = no_filter ? -1 : lv + hi;
  }
  return ORBFE_OK;
}

}  // namespace orbfe

extern "C" int orbfe_debug_last_claim_rounds(void) { return t_lastClaimRounds; }

extern "C" int orbfe_features_in_area(int device, const orbfe_frame_view* frame, int n_queries, const float* x,
                                      const float* y, const float* r, const int32_t* min_level,
                                      const int32_t* max_level, int capacity, int32_t* count, int32_t* indices) {
  frame = canon(frame);
  if (!frame_ok(frame) || n_queries < 0 || capacity < 0 ||
      (n_queries > 0 && (!x || !y || !r || !min_level || !max_level || !count || (capacity > 0 && !indices))))
    return fail(ORBFE_ERR_INVALID, "features_in_area: bad argument");
  if (n_queries == 0) return ORBFE_OK;
  WindowResult res;
  WindowJob job;
  job.f = frame; job.nq = n_queries; job.qx = x; job.qy = y; job.qr = r; job.qmin = min_level; job.qmax = max_level;
  job.res = &res;
  const int rc = window_search_multi(device, &job, 1, capacity);
  if (rc != ORBFE_OK) return rc;
  bool over = false;
  for (int i = 0; i < n_queries; i++) {
    count[i] = res.count[i];
    const int m = res.count[i] < capacity ? res.count[i] : capacity;
    if (res.count[i] > capacity) over = true;
    for (int c = 0; c < m; c++) indices[(size_t)i * capacity + c] = (int32_t)(res.cand[(size_t)i * res.K + c] & 0xffffu);
  }
  if (over) return fail(ORBFE_ERR_CAPACITY, "features_in_area: a window holds more features than capacity (counts are exact)");
  return ORBFE_OK;
}

extern "C" int orbfe_search_by_projection(int device, const orbfe_frame_view* F, const float* scale_factors,
                                          int n_levels, const uint8_t* blocked, int n_mp, const uint8_t* in_view,
                                          const int32_t* level, const float* view_cos, const float* proj_x,
                                          const float* proj_y, const float* proj_xr, const uint8_t* mp_desc,
                                          const uint8_t* mp_obs_positive, float th, float nnratio, int32_t* match,
                                          int32_t* n_matches) {
  F = canon(F);
  if (!frame_ok(F) || !scale_factors || n_levels <= 0 || n_mp < 0 || !n_matches || (F->n > 0 && (!match || !F->desc)) ||
      (n_mp > 0 && (!in_view || !level || !view_cos || !proj_x || !proj_y || !mp_desc)) || (F->u_right && n_mp > 0 && !proj_xr))
    return fail(ORBFE_ERR_INVALID, "search_by_projection: bad argument");
  for (int i = 0; i < n_mp; i++)
    if (in_view[i] && (level[i] < 0 || level[i] >= n_levels))
      return fail(ORBFE_ERR_INVALID, "search_by_projection: predicted level outside the pyramid");
  for (int i = 0; i < F->n; i++) match[i] = -1;
  *n_matches = 0;
  if (n_mp == 0 || F->n == 0) return ORBFE_OK;
  const bool bFactor = th != 1.0;
  std::vector<float> qr(n_mp);
  std::vector<int32_t> qmin(n_mp), qmax(n_mp);
  for (int i = 0; i < n_mp; i++) {
    float r = view_cos[i] > 0.998 ? 2.5f : 4.0f;  // RadiusByViewingCos, src/ORBmatcher.cc:140-146
    if (bFactor) r *= th;
    const int lv = in_view[i] ? level[i] : 0;
    qr[i] = r * scale_factors[lv];
    qmin[i] = lv - 1;
    qmax[i] = lv;
  }
  // the claim loop (:77-135: best / second best among the features no earlier map point holds, level + ratio test) runs on
  // the device behind the window search (k_window_claim); the match array comes back
  ClaimSpec C;
  C.mode = CLAIM_RATIO; C.maxDist = 100 /* TH_HIGH */; C.nnratio = nnratio;
  C.blocked = blocked; C.blockVal = mp_obs_positive;
  C.match = match; C.nMatches = n_matches;
  WindowJob job;
  job.f = F; job.nq = n_mp; job.qx = proj_x; job.qy = proj_y; job.qr = qr.data(); job.qmin = qmin.data(); job.qmax = qmax.data();
  job.qactive = in_view; job.qur = proj_xr; job.qdesc = mp_desc;
  job.claim = &C;
  return window_search_multi(device, &job, 1, 32);
}

extern "C" int orbfe_search_by_projection_last_frame(int device, const orbfe_frame_view* Cur, const float* scale_factors,
                                                     int n_levels, float mbf, int n_last, const uint8_t* valid,
                                                     const float* u, const float* v, const float* invzc,
                                                     const int32_t* last_octave, const float* last_angle,
                                                     const uint8_t* mp_desc, const uint8_t* obs_positive,
                                                     const uint8_t* blocked, int mode,
                                                     float th, int check_orientation, int32_t* match_cur,
                                                     int32_t* n_matches) {
  Cur = canon(Cur);
  if (!frame_ok(Cur) || !scale_factors || n_levels <= 0 || n_last < 0 || !n_matches || mode < 0 || mode > 2 ||
      (Cur->n > 0 && (!match_cur || !Cur->desc)) || (check_orientation && Cur->n > 0 && !Cur->angle) ||
      (n_last > 0 && (!valid || !u || !v || !last_octave || !mp_desc || (check_orientation && !last_angle))) ||
      (Cur->u_right && n_last > 0 && !invzc))
    return fail(ORBFE_ERR_INVALID, "search_by_projection_last_frame: bad argument");
  for (int i = 0; i < n_last; i++)
    if (valid[i] && (last_octave[i] < 0 || last_octave[i] >= n_levels))
      return fail(ORBFE_ERR_INVALID, "search_by_projection_last_frame: octave outside the pyramid");
  for (int i = 0; i < Cur->n; i++) match_cur[i] = -1;
  *n_matches = 0;
  if (n_last == 0 || Cur->n == 0) return ORBFE_OK;
  std::vector<float> qr(n_last), qur;
  std::vector<int32_t> qmin(n_last), qmax(n_last);
  if (Cur->u_right) qur.resize(n_last);
  for (int i = 0; i < n_last; i++) {
    const int o = valid[i] ? last_octave[i] : 0;
    qr[i] = th * scale_factors[o];  // src/ORBmatcher.cc:1543
    if (mode == 1) { qmin[i] = o; qmax[i] = -1; }            // bForward:  GetFeaturesInArea(u,v,radius,nLastOctave)
    else if (mode == 2) { qmin[i] = 0; qmax[i] = o; }        // bBackward: (u,v,radius,0,nLastOctave)
    else { qmin[i] = o - 1; qmax[i] = o + 1; }
    if (Cur->u_right) qur[i] = u[i] - mbf * invzc[i];        // :1562
  }
  ClaimSpec C = last_frame_claim(blocked, obs_positive, last_angle, check_orientation, match_cur, n_matches);
  WindowJob job;
  job.f = Cur; job.nq = n_last; job.qx = u; job.qy = v; job.qr = qr.data(); job.qmin = qmin.data(); job.qmax = qmax.data();
  job.qactive = valid; job.qur = Cur->u_right ? qur.data() : nullptr; job.qdesc = mp_desc;
  job.claim = &C;
  return window_search_multi(device, &job, 1, 32);
}

extern "C" int orbfe_search_by_projection_keyframe(int device, const orbfe_frame_view* Cur, const float* scale_factors,
                                                   int n_levels, const uint8_t* blocked, int n, const uint8_t* valid,
                                                   const float* u, const float* v, const int32_t* level,
                                                   const float* kf_angle, const uint8_t* mp_desc, float th,
                                                   int orb_dist, int check_orientation, int32_t* match_cur,
                                                   int32_t* n_matches) {
  Cur = canon(Cur);
  if (!frame_ok(Cur) || !scale_factors || n_levels <= 0 || n < 0 || !n_matches ||
      (Cur->n > 0 && (!match_cur || !Cur->desc)) || (check_orientation && Cur->n > 0 && !Cur->angle) ||
      (n > 0 && (!valid || !u || !v || !level || !mp_desc || (check_orientation && !kf_angle))))
    return fail(ORBFE_ERR_INVALID, "search_by_projection_keyframe: bad argument");
  std::vector<float> qr;
  std::vector<int32_t> qmin, qmax;
  int rc = level_queries("search_by_projection_keyframe", n, valid, level, scale_factors, n_levels, th, -1, +1, false,
                         &qr, &qmin, &qmax);
  if (rc != ORBFE_OK) return rc;
  for (int i = 0; i < Cur->n; i++) match_cur[i] = -1;
  *n_matches = 0;
  if (n == 0 || Cur->n == 0) return ORBFE_OK;
  ClaimSpec C = keyframe_claim(blocked, kf_angle, orb_dist, check_orientation, match_cur, n_matches);
  WindowJob job;
  job.f = Cur; job.nq = n; job.qx = u; job.qy = v; job.qr = qr.data(); job.qmin = qmin.data(); job.qmax = qmax.data();
  job.qactive = valid; job.qdesc = mp_desc;
  job.claim = &C;
  return window_search_multi(device, &job, 1, 32);
}

// The same search of ONE current frame against the projected map points of K candidate key frames in one call
// (Tracking::Relocalization, src/Tracking.cc:1577,1595: matcher2.SearchByProjection(mCurrentFrame, vpCandidateKFs[i],
// sFound, 10 | 3, 100 | 64) per candidate whose PnP pose survived).  Candidate k brings n[k] points: valid[k] / u[k] / v[k]
// / level[k] / kf_angle[k] / mp_desc[k] / blocked[k] (may be NULL) are its arrays; th[k] / orb_dist[k] its window and
// distance bound.  The K window searches share ONE upload of the queries, one launch group and one download
// (window_search_multi); a resident Cur uploads nothing of the frame.  match_cur [k * Cur->n + i2], n_matches [k].
extern "C" int orbfe_search_by_projection_keyframe_multi(int device, const orbfe_frame_view* Cur, const float* scale_factors,
                                                         int n_levels, int n_candidates, const uint8_t* const* blocked,
                                                         const int32_t* n, const uint8_t* const* valid, const float* const* u,
                                                         const float* const* v, const int32_t* const* level,
                                                         const float* const* kf_angle, const uint8_t* const* mp_desc,
                                                         const float* th, const int32_t* orb_dist, int check_orientation,
                                                         int32_t* match_cur, int32_t* n_matches) {
  Cur = canon(Cur);
  const int K = n_candidates;
  if (!frame_ok(Cur) || !scale_factors || n_levels <= 0 || K < 0 ||
      (K > 0 && (!n || !valid || !u || !v || !level || !mp_desc || !th || !orb_dist || !n_matches || (check_orientation && !kf_angle))) ||
      (Cur->n > 0 && K > 0 && (!match_cur || !Cur->desc)) || (check_orientation && Cur->n > 0 && !Cur->angle))
    return fail(ORBFE_ERR_INVALID, "search_by_projection_keyframe_multi: bad argument");
  std::vector<std::vector<float>> qr((size_t)K);
  std::vector<std::vector<int32_t>> qmin((size_t)K), qmax((size_t)K);
  std::vector<ClaimSpec> claims((size_t)K);
  std::vector<WindowJob> wj;
  for (int k = 0; k < K; k++) {
    if (n[k] < 0 || (n[k] > 0 && (!valid[k] || !u[k] || !v[k] || !level[k] || !mp_desc[k] || (check_orientation && !kf_angle[k]))))
      return fail(ORBFE_ERR_INVALID, "search_by_projection_keyframe_multi: NULL array of a candidate");
    int rc = level_queries("search_by_projection_keyframe_multi", n[k], valid[k], level[k], scale_factors, n_levels, th[k], -1, +1,
                           false, &qr[k], &qmin[k], &qmax[k]);
    if (rc != ORBFE_OK) return rc;
    for (int i = 0; i < Cur->n; i++) match_cur[(size_t)k * Cur->n + i] = -1;
    n_matches[k] = 0;
    if (n[k] == 0 || Cur->n == 0) continue;
    ClaimSpec& C = claims[k];
    C = keyframe_claim(blocked ? blocked[k] : nullptr, check_orientation ? kf_angle[k] : nullptr, orb_dist[k], check_orientation,
                       match_cur + (size_t)k * Cur->n, &n_matches[k]);
    WindowJob job;
    job.f = Cur; job.nq = n[k]; job.qx = u[k]; job.qy = v[k]; job.qr = qr[k].data(); job.qmin = qmin[k].data(); job.qmax = qmax[k].data();
    job.qactive = valid[k]; job.qdesc = mp_desc[k];
    job.claim = &C;
    wj.push_back(job);
  }
  if (wj.empty()) return ORBFE_OK;
  // one claim workgroup per candidate behind the K window searches: one upload, one launch group, one download
  return window_search_multi(device, wj.data(), (int)wj.size(), 32);
}

extern "C" int orbfe_search_by_projection_sim3(int device, const orbfe_frame_view* KF, const float* scale_factors,
                                               int n_levels, const uint8_t* matched, int n, const uint8_t* valid,
                                               const float* u, const float* v, const int32_t* level,
                                               const uint8_t* mp_desc, float th, int32_t* match, int32_t* n_matches) {
  KF = canon(KF);
  if (!frame_ok(KF) || !scale_factors || n_levels <= 0 || n < 0 || !n_matches || (KF->n > 0 && (!match || !KF->desc)) ||
      (n > 0 && (!valid || !u || !v || !level || !mp_desc)))
    return fail(ORBFE_ERR_INVALID, "search_by_projection_sim3: bad argument");
  std::vector<float> qr;
  std::vector<int32_t> qmin, qmax;
  // the reference gathers the window without a level filter and then keeps octaves [level-1, level]
  // (src/ORBmatcher.cc:410-428): the same set, in the same order, as filtering inside the window
  int rc = level_queries("search_by_projection_sim3", n, valid, level, scale_factors, n_levels, th, -1, 0, false, &qr,
                         &qmin, &qmax);
  if (rc != ORBFE_OK) return rc;
  for (int i = 0; i < KF->n; i++) match[i] = -1;
  *n_matches = 0;
  if (n == 0 || KF->n == 0) return ORBFE_OK;
  ClaimSpec C;  // claim loop :431-451 on the device
  C.mode = CLAIM_BEST; C.maxDist = 50 /* TH_LOW */;
  C.blocked = matched;
  C.match = match; C.nMatches = n_matches;
  WindowJob job;
  job.f = KF; job.nq = n; job.qx = u; job.qy = v; job.qr = qr.data(); job.qmin = qmin.data(); job.qmax = qmax.data();
  job.qactive = valid; job.qdesc = mp_desc;
  job.claim = &C;
  return window_search_multi(device, &job, 1, 32);
}

extern "C" int orbfe_search_for_initialization(int device, const orbfe_frame_view* F1, const orbfe_frame_view* F2,
                                               float* prev_x, float* prev_y, int window_size, float nnratio,
                                               int check_orientation, int32_t* match12, int32_t* n_matches) {
  F1 = canon(F1);
  F2 = canon(F2);
  if (!frame_ok(F1) || !frame_ok(F2) || !n_matches || window_size < 0 ||
      (F1->n > 0 && (!match12 || !prev_x || !prev_y || !F1->desc)) || (F2->n > 0 && !F2->desc) ||
      (check_orientation && ((F1->n > 0 && !F1->angle) || (F2->n > 0 && !F2->angle))))
    return fail(ORBFE_ERR_INVALID, "search_for_initialization: bad argument");
  const int n1 = F1->n;
  for (int i = 0; i < n1; i++) match12[i] = -1;
  *n_matches = 0;
  if (n1 == 0 || F2->n == 0) return ORBFE_OK;
  std::vector<float> qr(n1, (float)window_size);
  std::vector<int32_t> qlv(n1, 0);
  std::vector<uint8_t> active(n1);
  for (int i = 0; i < n1; i++) active[i] = F1->octave[i] > 0 ? 0 : 1;  // only level-0 keypoints (:482-484)
  for (int i = 0; i < n1; i++) qlv[i] = active[i] ? F1->octave[i] : 0;
  // the claim loop (:492-545: vMatchedDistance, the nnratio test, a later better match replaces the earlier one), the rotation
  // histogram (:557-563) and "update prev matched" (:595-600) run on the device (k_window_claim, CLAIM_INIT)
  ClaimSpec C;
  C.mode = CLAIM_INIT; C.maxDist = 50 /* TH_LOW */; C.nnratio = nnratio; C.checkOri = check_orientation ? 1 : 0;
  C.qAngle = F1->angle;
  C.match = match12; C.nMatches = n_matches;
  C.prevX = prev_x; C.prevY = prev_y;
  WindowJob job;
  job.f = F2; job.nq = n1; job.qx = prev_x; job.qy = prev_y; job.qr = qr.data(); job.qmin = qlv.data(); job.qmax = qlv.data();
  job.qactive = active.data(); job.qdesc = F1->desc;
  job.claim = &C;
  return window_search_multi(device, &job, 1, 128);
}

namespace {
// best keypoint of every window with octave in [level-1, level] (first minimum in scan order), the
// inner search shared by Fuse x2 and SearchBySim3; gate = chi-square test of Fuse (src/ORBmatcher.cc:1029-1060).
// Several (key frame, projected points) jobs of one call run as ONE window_search_multi group.
struct BestJob {
  const orbfe_frame_view* KF;
  const float* sf; const float* inv_level_sigma2;
  int n;
  const uint8_t* valid; const float *u, *v, *ur; const int32_t* level; const uint8_t* desc;
  int32_t* best;
};
int window_best_multi(const char* who, int device, BestJob* jobs, int nJobs, int n_levels, float th, bool gate, int max_dist) {
  std::vector<std::vector<float>> qr((size_t)nJobs);
  std::vector<std::vector<int32_t>> qmin((size_t)nJobs), qmax((size_t)nJobs);
  std::vector<WindowJob> wj;
  for (int j = 0; j < nJobs; j++) {
    BestJob& J = jobs[j];
    int rc = level_queries(who, J.n, J.valid, J.level, J.sf, n_levels, th, -1, 0, false, &qr[j], &qmin[j], &qmax[j]);
    if (rc != ORBFE_OK) return rc;
    for (int i = 0; i < J.n; i++) J.best[i] = -1;
    if (J.n == 0 || J.KF->n == 0) continue;
    // The whole inner search runs on the device (round 4): the window scan, the octave filter, Fuse's chi-square gate
    // (src/ORBmatcher.cc:1036-1058) and the first minimum with its distance bound -- a point's best keypoint depends on no
    // other point, so there is no claim loop to replay: 4 bytes per point come back instead of a 32-entry candidate list
    WindowJob w;
    w.f = J.KF; w.nq = J.n; w.qx = J.u; w.qy = J.v; w.qr = qr[j].data(); w.qmin = qmin[j].data(); w.qmax = qmax[j].data();
    w.qactive = J.valid; w.qdesc = J.desc;
    w.bestOut = J.best;
    w.gate = gate ? 1 : 0;
    w.gur = (gate && J.KF->u_right) ? J.ur : nullptr;
    w.invSigma2 = J.inv_level_sigma2;
    w.nLevels = n_levels;
    w.maxDist = max_dist;
    wj.push_back(w);
  }
  if (wj.empty()) return ORBFE_OK;
  return window_search_multi(device, wj.data(), (int)wj.size(), 8);
}
}  // namespace

// The per-point search of ORBmatcher::Fuse for the SAME map points against K key frames in one call: what
// LocalMapping::SearchInNeighbors does neighbour by neighbour (src/LocalMapping.cc:542-549: matcher.Fuse(pKFi,
// vpMapPointMatches) for every target key frame).  Arrays are [k * n + i]; mp_desc [n * 32] is shared.
extern "C" int orbfe_fuse_search_multi(int device, int n_keyframes, const orbfe_frame_view* const* KF,
                                       const float* scale_factors, const float* inv_level_sigma2, int n_levels, int n,
                                       const uint8_t* valid, const float* u, const float* v, const float* ur,
                                       const int32_t* level, const uint8_t* mp_desc, float th, int chi2_gate,
                                       int32_t* best_idx) {
  if (n_keyframes < 0 || n < 0 || !scale_factors || n_levels <= 0 || (n_keyframes > 0 && !KF) ||
      (n_keyframes > 0 && n > 0 && (!valid || !u || !v || !level || !mp_desc || !best_idx)) || (chi2_gate && !inv_level_sigma2))
    return fail(ORBFE_ERR_INVALID, "fuse_search_multi: bad argument");
  std::vector<BestJob> jobs;
  for (int k = 0; k < n_keyframes; k++) {
    const orbfe_frame_view* f = canon(KF[k]);
    if (!frame_ok(f) || (f->n > 0 && !f->desc) || (chi2_gate && f->u_right && n > 0 && !ur))
      return fail(ORBFE_ERR_INVALID, "fuse_search_multi: bad key frame view");
    for (int i = 0; i < f->n; i++)
      if (chi2_gate && (f->octave[i] < 0 || f->octave[i] >= n_levels))
        return fail(ORBFE_ERR_INVALID, "fuse_search_multi: keypoint octave outside the pyramid");
    const size_t o = (size_t)k * n;
    jobs.push_back(BestJob{f, scale_factors, inv_level_sigma2, n, valid + o, u + o, v + o, ur ? ur + o : nullptr, level + o,
                           mp_desc, best_idx + o});
  }
  if (jobs.empty()) return ORBFE_OK;
  return window_best_multi("fuse_search_multi", device, jobs.data(), (int)jobs.size(), n_levels, th, chi2_gate != 0, 50 /* TH_LOW */);
}

extern "C" int orbfe_fuse_search(int device, const orbfe_frame_view* KF, const float* scale_factors,
                                 const float* inv_level_sigma2, int n_levels, int n, const uint8_t* valid,
                                 const float* u, const float* v, const float* ur, const int32_t* level,
                                 const uint8_t* mp_desc, float th, int chi2_gate, int32_t* best_idx) {
  KF = canon(KF);
  if (!frame_ok(KF) || !scale_factors || n_levels <= 0 || n < 0 || (KF->n > 0 && !KF->desc) ||
      (n > 0 && (!valid || !u || !v || !level || !mp_desc || !best_idx)) ||
      (chi2_gate && (!inv_level_sigma2 || (KF->u_right && n > 0 && !ur))))
    return fail(ORBFE_ERR_INVALID, "fuse_search: bad argument");
  for (int i = 0; i < KF->n; i++)
    if (chi2_gate && (KF->octave[i] < 0 || KF->octave[i] >= n_levels))
      return fail(ORBFE_ERR_INVALID, "fuse_search: keypoint octave outside the pyramid");
  BestJob job{KF, scale_factors, inv_level_sigma2, n, valid, u, v, ur, level, mp_desc, best_idx};
  return window_best_multi("fuse_search", device, &job, 1, n_levels, th, chi2_gate != 0, 50 /* TH_LOW */);
}

extern "C" int orbfe_search_by_sim3(int device, const orbfe_frame_view* KF1, const orbfe_frame_view* KF2,
                                    const float* scale_factors1, const float* scale_factors2, int n_levels,
                                    const uint8_t* valid1, const float* u1, const float* v1, const int32_t* level1,
                                    const uint8_t* desc1, const uint8_t* valid2, const float* u2, const float* v2,
                                    const int32_t* level2, const uint8_t* desc2, float th, int32_t* match12,
                                    int32_t* n_found) {
  KF1 = canon(KF1);
  KF2 = canon(KF2);
  if (!frame_ok(KF1) || !frame_ok(KF2) || !scale_factors1 || !scale_factors2 || n_levels <= 0 || !n_found ||
      (KF1->n > 0 && (!valid1 || !u1 || !v1 || !level1 || !desc1 || !match12 || !KF1->desc)) ||
      (KF2->n > 0 && (!valid2 || !u2 || !v2 || !level2 || !desc2 || !KF2->desc)))
    return fail(ORBFE_ERR_INVALID, "search_by_sim3: bad argument");
  std::vector<int32_t> m1(KF1->n ? KF1->n : 1), m2(KF2->n ? KF2->n : 1);
  // both directions (src/ORBmatcher.cc:1190-1275 and :1277-1358) as one upload / launch group / download
  BestJob jobs[2] = {{KF2, scale_factors2, nullptr, KF1->n, valid1, u1, v1, nullptr, level1, desc1, m1.data()},
                     {KF1, scale_factors1, nullptr, KF2->n, valid2, u2, v2, nullptr, level2, desc2, m2.data()}};
  int rc = window_best_multi("search_by_sim3", device, jobs, 2, n_levels, th, false, 100 /* TH_HIGH */);
  if (rc != ORBFE_OK) return rc;
  int nFound = 0;
  for (int i1 = 0; i1 < KF1->n; i1++) {
    match12[i1] = -1;
    const int idx2 = m1[i1];
    if (idx2 >= 0 && m2[idx2] == i1) { match12[i1] = idx2; nFound++; }
  }
  *n_found = nFound;
  return ORBFE_OK;
}
