// pnp.hip -- C-ABI entry points of PnPsolver (include/orbfe.h, "PnPsolver").  orbfe_pnp_ransac* and orbfe_pnp_refine_multi
// are one staged copy up, ONE launch (k_pnp.hip) and one copy back on the calling thread's matcher stream, complete on
// return; orbfe_pnp_solve_multi makes that round trip once per launch with the record scan between them.  The argument
// checks, the layouts and the pure host functions are pnp_host.h (no device needed).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "pnp_host.h"
#include "pnp_kernels.h"

using namespace orbfe;

namespace {

struct Points {
  int K, N;
  const int32_t* point_off;
  const float *p3d, *p2d, *max_err2, *cam;
};
struct Results {
  int32_t* n_inliers;
  uint8_t* status;
  float* pose;
  int32_t* word_off;
  uint32_t* mask_words;
};

// one round trip: `I` items (hypotheses with `sets`, or records with idxOff / idx), already checked
int round_trip(int device, const Points& P, int I, const int32_t* item_off, const int32_t* sets,
               const std::vector<int32_t>* idxOff, const std::vector<int32_t>* idx, const Results& O) {
  std::vector<PnpCandidate> cands;
  std::vector<int32_t> itemCand;
  pnp_layout(P.K, P.point_off, item_off, P.cam, O.word_off, &cands, &itemCand);
  if (I == 0) return ORBFE_OK;
  const size_t words = (size_t)O.word_off[P.K];

  PnpArgs A = {};
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    PnpCandidate* dc;
    int32_t *dh, *ds = nullptr, *dio = nullptr, *di = nullptr;
    float *d3, *d2, *de;
    TRY(up(a, &dc, cands.data(), cands.size()));
    TRY(up(a, &dh, itemCand.data(), itemCand.size()));
    if (sets) {
      TRY(up(a, &ds, sets, (size_t)I * 4));
    } else {
      TRY(up(a, &dio, idxOff->data(), idxOff->size()));
      TRY(up(a, &di, idx->data(), idx->size()));
    }
    TRY(up(a, &d3, P.p3d, (size_t)P.N * 3));
    TRY(up(a, &d2, P.p2d, (size_t)P.N * 2));
    TRY(up(a, &de, P.max_err2, (size_t)P.N));
    open_span(a);  // the four outputs adjacent: one copy back; the kernel writes every element
    A.nInliers = carve<int32_t>(a, (size_t)I);
    A.pose = carve<float>(a, (size_t)I * 12);
    A.words = carve<uint32_t>(a, words ? words : 1);
    A.status = carve<uint8_t>(a, (size_t)I);
    TRY(close_span(a));
    A.nItems = I;
    A.cands = dc; A.itemCand = dh; A.sets = ds; A.idxOff = dio; A.idx = di;
    A.p3d = d3; A.p2d = d2; A.maxErr2 = de;
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  if (sets) launch_pnp_ransac(ar->stream, A);
  else launch_pnp_refine(ar->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(O.n_inliers, mirror_of(ar, A.nInliers), (size_t)I * 4);
  std::memcpy(O.pose, mirror_of(ar, A.pose), (size_t)I * 12 * sizeof(float));
  if (words) std::memcpy(O.mask_words, mirror_of(ar, A.words), words * 4);
  std::memcpy(O.status, mirror_of(ar, A.status), (size_t)I);
  return ORBFE_OK;
}

int ransac(const char* who, int device, const Points& P, int H, const int32_t* hyp_off, const int32_t* sets, const Results& O) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, std::string(who) + ": negative device");
  const char* e = pnp_check_common(P.K, P.N, H, P.point_off, P.p3d, P.p2d, P.max_err2, P.cam, hyp_off, sets, O.n_inliers, O.status,
                                   O.pose, O.word_off, O.mask_words);
  if (!e && H > 0) e = pnp_check_sets(P.K, P.point_off, hyp_off, sets);
  if (e) return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  return round_trip(device, P, H, hyp_off, sets, nullptr, nullptr, O);
}

int refine(const char* who, int device, const Points& P, int R, const int32_t* rec_off, const uint32_t* rec_masks,
           const Results& O) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, std::string(who) + ": negative device");
  const char* e = pnp_check_common(P.K, P.N, R, P.point_off, P.p3d, P.p2d, P.max_err2, P.cam, rec_off, rec_masks, O.n_inliers,
                                   O.status, O.pose, O.word_off, O.mask_words);
  if (!e && R > 0) e = pnp_check_masks(P.K, P.point_off, rec_off, rec_masks);
  if (e) return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  std::vector<int32_t> idxOff, idx;
  pnp_compact(P.K, P.point_off, rec_off, rec_masks, &idxOff, &idx);
  return round_trip(device, P, R, rec_off, nullptr, &idxOff, &idx, O);
}

}  // namespace

extern "C" int orbfe_pnp_ransac_multi(int device, int n_candidates, int n_points, int n_hypotheses, const int32_t* point_off,
                                      const float* p3d, const float* p2d, const float* max_err2, const float* cam,
                                      const int32_t* hyp_off, const int32_t* sets, int32_t* n_inliers, uint8_t* status, float* pose,
                                      int32_t* word_off, uint32_t* mask_words) {
  const Points P = {n_candidates, n_points, point_off, p3d, p2d, max_err2, cam};
  return ransac("pnp_ransac_multi", device, P, n_hypotheses, hyp_off, sets, Results{n_inliers, status, pose, word_off, mask_words});
}

extern "C" int orbfe_pnp_ransac(int device, int n_points, const float* p3d, const float* p2d, const float* max_err2,
                                const float* cam, int n_hypotheses, const int32_t* sets, int32_t* n_inliers, uint8_t* status,
                                float* pose, uint32_t* mask_words) {
  const int32_t pointOff[2] = {0, n_points}, hypOff[2] = {0, n_hypotheses};
  int32_t wordOff[2];
  const Points P = {1, n_points, pointOff, p3d, p2d, max_err2, cam};
  return ransac("pnp_ransac", device, P, n_hypotheses, hypOff, sets, Results{n_inliers, status, pose, wordOff, mask_words});
}

extern "C" int orbfe_pnp_refine_multi(int device, int n_candidates, int n_points, int n_records, const int32_t* point_off,
                                      const float* p3d, const float* p2d, const float* max_err2, const float* cam,
                                      const int32_t* rec_off, const uint32_t* rec_masks, int32_t* n_inliers, uint8_t* status,
                                      float* pose, int32_t* word_off, uint32_t* mask_words) {
  const Points P = {n_candidates, n_points, point_off, p3d, p2d, max_err2, cam};
  return refine("pnp_refine_multi", device, P, n_records, rec_off, rec_masks, Results{n_inliers, status, pose, word_off, mask_words});
}

extern "C" int orbfe_pnp_solve_multi(int device, int n_candidates, int n_points, int n_hypotheses, const int32_t* point_off,
                                     const float* p3d, const float* p2d, const float* max_err2, const float* cam,
                                     const int32_t* hyp_off, const int32_t* sets, const int32_t* min_inliers, int32_t* n_inliers,
                                     uint8_t* status, float* pose, int32_t* word_off, uint32_t* mask_words, int32_t* rec_off,
                                     int32_t* rec_hyp, int32_t* rec_n_inliers, uint8_t* rec_status, float* rec_pose,
                                     int32_t* rec_word_off, uint32_t* rec_mask_words) {
  const char* who = "pnp_solve_multi";
  const int K = n_candidates, H = n_hypotheses;
  if (const char* e = pnp_check_solve(K, H, min_inliers, rec_off, rec_hyp, rec_n_inliers, rec_status, rec_pose, rec_word_off,
                                      rec_mask_words))
    return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  const Points P = {K, n_points, point_off, p3d, p2d, max_err2, cam};
  int rc = ransac(who, device, P, H, hyp_off, sets, Results{n_inliers, status, pose, word_off, mask_words});
  if (rc != ORBFE_OK) return rc;
  std::vector<int32_t> recHyp;
  pnp_scan_records(K, hyp_off, n_inliers, min_inliers, rec_off, &recHyp);
  std::vector<uint32_t> masks;  // the records' masks are the hypotheses' own words
  for (int k = 0; k < K; k++) {
    const size_t words = (size_t)((point_off[k + 1] - point_off[k] + 31) / 32);
    for (int r = rec_off[k]; r < rec_off[k + 1]; r++) {
      const uint32_t* w = mask_words + (size_t)word_off[k] + (size_t)(recHyp[r] - hyp_off[k]) * words;
      masks.insert(masks.end(), w, w + words);
    }
  }
  const int R = (int)recHyp.size();
  if (R) std::memcpy(rec_hyp, recHyp.data(), (size_t)R * 4);
  return refine(who, device, P, R, rec_off, masks.data(), Results{rec_n_inliers, rec_status, rec_pose, rec_word_off, rec_mask_words});
}

extern "C" int orbfe_pnp_sets_from_draws(int n, int n_hypotheses, const int32_t* draws, int32_t* sets) {
  if (!pnp_sets_from_draws(n, n_hypotheses, draws, sets))
    return fail(ORBFE_ERR_INVALID, "pnp_sets_from_draws: fewer than 4 correspondences, a NULL array or a draw outside [0, n - 1 - i]");
  return ORBFE_OK;
}
