// initializer.hip -- C-ABI entry points of the Initializer H/F RANSAC evaluation (include/orbfe.h, "Initializer").  A call is
// one staged copy up, ONE launch of k_initializer (k_initializer.hip) and one copy back on the calling thread's matcher stream,
// complete on return.  The argument checks, the layout and the two pure host functions are initializer_host.h (no device
// needed).  orbfe_initializer_reconstruct* (ReconstructH / ReconstructF with CheckRT) are staged the same way around ONE
// launch of k_init_reconstruct (k_init_reconstruct.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "initializer_host.h"
#include "initializer_kernels.h"

using namespace orbfe;

namespace {

int run(const char* who, int device, int K, int N, int H, const int32_t* pair_off, const float* pairs, const double* T1,
        const double* T2, const float* sigma, const int32_t* hyp_off, const int32_t* sets, double* score, uint8_t* status,
        int32_t* n_inliers, double* model, double* h12, uint32_t* mask_words, int32_t* word_off) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, std::string(who) + ": negative device");
  if (const char* e = init_check(K, N, H, pair_off, pairs, T1, T2, sigma, hyp_off, sets, score, status, n_inliers, model, h12,
                                 mask_words, word_off))
    return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  std::vector<InitProblem> probs;
  std::vector<int32_t> hypProb;
  init_layout(K, pair_off, hyp_off, T1, T2, sigma, word_off, &probs, &hypProb);
  if (H == 0) return ORBFE_OK;
  const size_t words = (size_t)word_off[K];

  InitArgs A = {};
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    InitProblem* dp;
    int32_t *dh, *ds;
    float* dx;
    TRY(up(a, &dp, probs.data(), probs.size()));
    TRY(up(a, &dh, hypProb.data(), hypProb.size()));
    TRY(up(a, &ds, sets, (size_t)H * 8));
    TRY(up(a, &dx, pairs, (size_t)N * 4));
    open_span(a);  // the outputs adjacent: one copy back; the kernel writes every element
    A.score = carve<double>(a, (size_t)H * 2);
    A.model = carve<double>(a, (size_t)H * 18);
    A.h12 = carve<double>(a, (size_t)H * 9);
    A.nInliers = carve<int32_t>(a, (size_t)H * 2);
    A.words = carve<uint32_t>(a, words ? words : 1);
    A.status = carve<uint8_t>(a, (size_t)H * 2);
    TRY(close_span(a));
    A.nHyp = H;
    A.probs = dp; A.hypProb = dh; A.sets = ds; A.pairs = dx;
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_initializer(ar->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(score, mirror_of(ar, A.score), (size_t)H * 2 * sizeof(double));
  std::memcpy(model, mirror_of(ar, A.model), (size_t)H * 18 * sizeof(double));
  std::memcpy(h12, mirror_of(ar, A.h12), (size_t)H * 9 * sizeof(double));
  std::memcpy(n_inliers, mirror_of(ar, A.nInliers), (size_t)H * 2 * 4);
  if (words) std::memcpy(mask_words, mirror_of(ar, A.words), words * 4);
  std::memcpy(status, mirror_of(ar, A.status), (size_t)H * 2);
  return ORBFE_OK;
}

// orbfe_initializer_reconstruct*: one staged copy up, ONE launch of k_init_reconstruct and one copy back
int run_reconstruct(const char* who, int device, int K, int N, int W, const int32_t* pair_off, const float* pairs,
                    const int32_t* model_kind, const double* model, const float* K4, const float* sigma,
                    const uint32_t* inlier_words, const int32_t* in_word_off, int32_t* hyp_off, int32_t* slot_off, double* R,
                    double* t, int32_t* n_good, double* cos_sel, uint8_t* hyp_status, double* x3d, uint8_t* pair_flags,
                    uint8_t* problem_status, int32_t* n_inliers) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, std::string(who) + ": negative device");
  if (const char* e = recon_check(K, N, W, pair_off, pairs, model_kind, model, K4, sigma, inlier_words, in_word_off, hyp_off,
                                  slot_off, R, t, n_good, cos_sel, hyp_status, x3d, pair_flags, problem_status, n_inliers))
    return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  std::vector<ReconProblem> probs;
  std::vector<int32_t> hypProb;
  recon_layout(K, pair_off, model_kind, model, K4, sigma, in_word_off, hyp_off, slot_off, &probs, &hypProb);
  if (K == 0) return ORBFE_OK;
  const size_t G = (size_t)hyp_off[K], slots = (size_t)slot_off[K];

  ReconArgs A = {};
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    ReconProblem* dp;
    int32_t* dh;
    float* dx;
    uint32_t* dw;
    TRY(up(a, &dp, probs.data(), probs.size()));
    TRY(up(a, &dh, hypProb.data(), hypProb.size()));
    TRY(up(a, &dx, pairs, (size_t)N * 4));
    TRY(up(a, &dw, inlier_words, (size_t)W));
    A.keys = carve<uint64_t>(a, slots ? slots : 1);
    open_span(a);  // the outputs adjacent: one copy back; the kernel writes every element
    A.R = carve<double>(a, G * 9);
    A.t = carve<double>(a, G * 3);
    A.cosSel = carve<double>(a, G);
    A.x3d = carve<double>(a, slots ? slots * 3 : 1);
    A.nGood = carve<int32_t>(a, G);
    A.nInliers = carve<int32_t>(a, (size_t)K);
    A.hypStatus = carve<uint8_t>(a, G);
    A.pairFlags = carve<uint8_t>(a, slots ? slots : 1);
    A.problemStatus = carve<uint8_t>(a, (size_t)K);
    TRY(close_span(a));
    A.nHyp = (int)G;
    A.probs = dp; A.hypProb = dh; A.pairs = dx; A.words = dw;
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_init_reconstruct(ar->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  std::memcpy(R, mirror_of(ar, A.R), G * 9 * sizeof(double));
  std::memcpy(t, mirror_of(ar, A.t), G * 3 * sizeof(double));
  std::memcpy(cos_sel, mirror_of(ar, A.cosSel), G * sizeof(double));
  if (slots) std::memcpy(x3d, mirror_of(ar, A.x3d), slots * 3 * sizeof(double));
  std::memcpy(n_good, mirror_of(ar, A.nGood), G * 4);
  std::memcpy(n_inliers, mirror_of(ar, A.nInliers), (size_t)K * 4);
  std::memcpy(hyp_status, mirror_of(ar, A.hypStatus), G);
  if (slots) std::memcpy(pair_flags, mirror_of(ar, A.pairFlags), slots);
  std::memcpy(problem_status, mirror_of(ar, A.problemStatus), (size_t)K);
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_initializer_reconstruct_multi(int device, int n_problems, int n_pairs, int n_words, const int32_t* pair_off,
                                                   const float* pairs, const int32_t* model_kind, const double* model,
                                                   const float* K4, const float* sigma, const uint32_t* inlier_words,
                                                   const int32_t* in_word_off, int32_t* hyp_off, int32_t* slot_off, double* R,
                                                   double* t, int32_t* n_good, double* cos_sel, uint8_t* hyp_status, double* x3d,
                                                   uint8_t* pair_flags, uint8_t* problem_status, int32_t* n_inliers) {
  return run_reconstruct("initializer_reconstruct_multi", device, n_problems, n_pairs, n_words, pair_off, pairs, model_kind, model,
                         K4, sigma, inlier_words, in_word_off, hyp_off, slot_off, R, t, n_good, cos_sel, hyp_status, x3d, pair_flags,
                         problem_status, n_inliers);
}

extern "C" int orbfe_initializer_reconstruct(int device, int n_pairs, const float* pairs, int model_kind, const double* model,
                                             const float* K4, float sigma, const uint32_t* inlier_words, double* R, double* t,
                                             int32_t* n_good, double* cos_sel, uint8_t* hyp_status, double* x3d,
                                             uint8_t* pair_flags, uint8_t* problem_status, int32_t* n_inliers) {
  if (n_pairs < 0 || n_pairs > INT32_MAX - 31) return fail(ORBFE_ERR_INVALID, "initializer_reconstruct: n_pairs outside [0, 2^31 - 32]");
  const int32_t words = (n_pairs + 31) / 32, kind = model_kind;
  const int32_t pairOff[2] = {0, n_pairs}, wordOff[2] = {0, words};
  int32_t hypOff[2], slotOff[2];
  return run_reconstruct("initializer_reconstruct", device, 1, n_pairs, words, pairOff, pairs, &kind, model, K4, &sigma,
                         inlier_words, wordOff, hypOff, slotOff, R, t, n_good, cos_sel, hyp_status, x3d, pair_flags,
                         problem_status, n_inliers);
}

extern "C" int orbfe_initializer_ransac_multi(int device, int n_problems, int n_pairs, int n_sets, const int32_t* pair_off,
                                              const float* pairs, const double* T1, const double* T2, const float* sigma,
                                              const int32_t* hyp_off, const int32_t* sets, double* score, uint8_t* status,
                                              int32_t* n_inliers, double* model, double* h12, uint32_t* mask_words,
                                              int32_t* word_off) {
  return run("initializer_ransac_multi", device, n_problems, n_pairs, n_sets, pair_off, pairs, T1, T2, sigma, hyp_off, sets, score,
             status, n_inliers, model, h12, mask_words, word_off);
}

extern "C" int orbfe_initializer_ransac(int device, int n_pairs, const float* pairs, const double* T1, const double* T2,
                                        float sigma, int n_sets, const int32_t* sets, double* score, uint8_t* status,
                                        int32_t* n_inliers, double* model, double* h12, uint32_t* mask_words) {
  const int32_t pairOff[2] = {0, n_pairs}, hypOff[2] = {0, n_sets};
  int32_t wordOff[2];
  return run("initializer_ransac", device, 1, n_pairs, n_sets, pairOff, pairs, T1, T2, &sigma, hypOff, sets, score, status,
             n_inliers, model, h12, mask_words, wordOff);
}

extern "C" int orbfe_initializer_normalize(int n_keys, const float* keys_xy, double* T) {
  if (!init_normalize(n_keys, keys_xy, T)) return fail(ORBFE_ERR_INVALID, "initializer_normalize: no keys or a NULL array");
  return ORBFE_OK;
}

extern "C" int orbfe_initializer_sets_from_draws(int n, int n_sets, const int32_t* draws, int32_t* sets) {
  if (!init_sets_from_draws(n, n_sets, draws, sets))
    return fail(ORBFE_ERR_INVALID, "initializer_sets_from_draws: fewer than 8 pairs, a NULL array or a draw outside [0, n - j)");
  return ORBFE_OK;
}
