// sim3.hip -- C-ABI entry points of the Sim3 RANSAC evaluation (include/orbfe.h, "Sim3Solver").  A call is one staged copy
// up, ONE launch of k_sim3 (k_sim3.hip) and one copy back on the calling thread's matcher stream, complete on return.  The
// argument checks, the layout and the two pure host functions are sim3_host.h (no device needed).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "sim3_host.h"
#include "sim3_kernels.h"

using namespace orbfe;

namespace {

int run(const char* who, int device, int K, int N, int H, const int32_t* pair_off, const float* x3dc1, const float* x3dc2,
        const float* max_err1, const float* max_err2, const float* cam1, const float* cam2, int fix_scale,
        const int32_t* hyp_off, const int32_t* triples, int32_t* n_inliers, uint8_t* status, float* sim3, uint32_t* mask_words,
        int32_t* word_off) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, std::string(who) + ": negative device");
  if (const char* e = sim3_check(K, N, H, pair_off, x3dc1, x3dc2, max_err1, max_err2, cam1, cam2, hyp_off, triples, n_inliers,
                                 status, sim3, mask_words, word_off))
    return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  std::vector<Sim3Candidate> cands;
  std::vector<int32_t> hypCand;
  sim3_layout(K, pair_off, hyp_off, cam1, cam2, word_off, &cands, &hypCand);
  if (H == 0) return ORBFE_OK;
  const size_t words = (size_t)word_off[K];

  Sim3Args A = {};
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    Sim3Candidate* dc;
    int32_t *dh, *dt;
    float *d1, *d2, *e1, *e2;
    TRY(up(a, &dc, cands.data(), cands.size()));
    TRY(up(a, &dh, hypCand.data(), hypCand.size()));
    TRY(up(a, &dt, triples, (size_t)H * 3));
    TRY(up(a, &d1, x3dc1, (size_t)N * 3));
    TRY(up(a, &d2, x3dc2, (size_t)N * 3));
    TRY(up(a, &e1, max_err1, (size_t)N));
    TRY(up(a, &e2, max_err2, (size_t)N));
    open_span(a);  // the four outputs adjacent: one copy back; the kernel writes every element
    A.nInliers = carve<int32_t>(a, (size_t)H);
    A.sim3 = carve<float>(a, (size_t)H * 13);
    A.words = carve<uint32_t>(a, words ? words : 1);
    A.status = carve<uint8_t>(a, (size_t)H);
    TRY(close_span(a));
    A.nHyp = H; A.fixScale = fix_scale ? 1 : 0;
    A.cands = dc; A.hypCand = dh; A.triples = dt;
    A.x3dc1 = d1; A.x3dc2 = d2; A.maxErr1 = e1; A.maxErr2 = e2;
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_sim3(ar->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(n_inliers, mirror_of(ar, A.nInliers), (size_t)H * 4);
  std::memcpy(sim3, mirror_of(ar, A.sim3), (size_t)H * 13 * sizeof(float));
  if (words) std::memcpy(mask_words, mirror_of(ar, A.words), words * 4);
  std::memcpy(status, mirror_of(ar, A.status), (size_t)H);
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_sim3_ransac_multi(int device, int n_candidates, int n_pairs, int n_hypotheses, const int32_t* pair_off,
                                       const float* x3dc1, const float* x3dc2, const float* max_err1, const float* max_err2,
                                       const float* cam1, const float* cam2, int fix_scale, const int32_t* hyp_off,
                                       const int32_t* triples, int32_t* n_inliers, uint8_t* status, float* sim3,
                                       uint32_t* mask_words, int32_t* word_off) {
  return run("sim3_ransac_multi", device, n_candidates, n_pairs, n_hypotheses, pair_off, x3dc1, x3dc2, max_err1, max_err2, cam1,
             cam2, fix_scale, hyp_off, triples, n_inliers, status, sim3, mask_words, word_off);
}

extern "C" int orbfe_sim3_ransac(int device, int n_pairs, const float* x3dc1, const float* x3dc2, const float* max_err1,
                                 const float* max_err2, const float* cam1, const float* cam2, int fix_scale, int n_hypotheses,
                                 const int32_t* triples, int32_t* n_inliers, uint8_t* status, float* sim3, uint32_t* mask_words) {
  const int32_t pairOff[2] = {0, n_pairs}, hypOff[2] = {0, n_hypotheses};
  int32_t wordOff[2];
  return run("sim3_ransac", device, 1, n_pairs, n_hypotheses, pairOff, x3dc1, x3dc2, max_err1, max_err2, cam1, cam2, fix_scale,
             hypOff, triples, n_inliers, status, sim3, mask_words, wordOff);
}

extern "C" int orbfe_sim3_triples_from_draws(int n, int n_hypotheses, const int32_t* draws, int32_t* triples) {
  if (!sim3_triples_from_draws(n, n_hypotheses, draws, triples))
    return fail(ORBFE_ERR_INVALID, "sim3_triples_from_draws: fewer than 3 pairs, a NULL array or a draw outside [0, n - 1 - i]");
  return ORBFE_OK;
}

extern "C" int orbfe_sim3_max_iterations(int n, double prob, int min_inliers, int max_its) {
  return sim3_max_iterations(n, prob, min_inliers, max_its);
}
