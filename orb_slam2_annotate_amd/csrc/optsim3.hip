// optsim3.hip -- C-ABI entry points of the Sim3 optimisation (include/orbfe.h, "Optimizer::OptimizeSim3").  A call is one
// staged copy up, ONE launch of k_optimize_sim3 (k_optsim3.hip) and one copy back on the calling thread's matcher stream
// (arena.h: arena_stage), complete on return.  The argument checks and the packing are optsim3_host.h (no device needed).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "../../include/orbfe.h"
#include "arena.h"
#include "host_internal.h"
#include "optsim3_host.h"
#include "optsim3_kernels.h"

using namespace orbfe;

namespace {

static_assert(kOptSim3HostMaxPairs == kOptSim3MaxPairs, "one per-problem limit");

int run_multi(int device, int K, const int32_t* pair_off, const float* x3dc1, const float* x3dc2, const float* obs1,
              const float* obs2, const float* w1, const float* w2, const float* cam1, const float* cam2, const float* sim3_in,
              const float* th2, const uint8_t* fix_scale, double* sim3_out, uint8_t* bad, int32_t* n_in,
              orbfe_optsim3_stats* stats, double* chi2_12, double* chi2_21) {
  if (K == 0) return ORBFE_OK;
  const int N = pair_off[K];
  const size_t n1 = (size_t)(N ? N : 1);
  OptSim3Args A{};
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    OptSim3Problem* dp;
    float4 *dA, *dB, *dC;
    TRY(up_pack(a, &dp, (size_t)K, [&](OptSim3Problem* h) { optsim3_pack_problems(h, K, pair_off, cam1, cam2, sim3_in, th2, fix_scale); }));
    TRY(up_pack(a, &dA, (size_t)N, [&](float4* h) { optsim3_pack_pairs_a(&h->x, N, x3dc1, w1); }));
    TRY(up_pack(a, &dB, (size_t)N, [&](float4* h) { optsim3_pack_pairs_b(&h->x, N, x3dc2, w2); }));
    TRY(up_pack(a, &dC, (size_t)N, [&](float4* h) { optsim3_pack_pairs_c(&h->x, N, obs1, obs2); }));
    A.prob = dp; A.pairA = dA; A.pairB = dB; A.pairC = dC;
    open_span(a);  // the four outputs adjacent: one copy back
    A.res = carve<OptSim3Result>(a, (size_t)K);
    A.bad = carve<uint8_t>(a, n1);
    A.chi12 = carve<double>(a, n1);
    A.chi21 = carve<double>(a, n1);
    return close_span(a);
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(flush(ar));
  launch_optimize_sim3(ar->stream, A, K);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  const OptSim3Result* hr = mirror_of(ar, A.res);
  const uint8_t* hb = mirror_of(ar, A.bad);
  const double* h12 = mirror_of(ar, A.chi12);
  const double* h21 = mirror_of(ar, A.chi21);
  for (int p = 0; p < K; p++) {
    std::memcpy(sim3_out + 8 * (size_t)p, hr[p].sim3, 8 * sizeof(double));
    n_in[p] = hr[p].nIn;
    if (stats) {
      orbfe_optsim3_stats* st = stats + p;
      st->rounds = hr[p].rounds; st->n_bad = hr[p].nBad;
      for (int r = 0; r < 2; r++) {
        st->iterations[r] = hr[p].iterations[r]; st->trials[r] = hr[p].trials[r];
        st->lambda[r] = hr[p].lambda[r]; st->chi2[r] = hr[p].chi2[r];
      }
    }
    const int off = pair_off[p], n = pair_off[p + 1] - off;
    if (n == 0) continue;
    std::memcpy(bad + off, hb + off, (size_t)n);
    if (chi2_12) std::memcpy(chi2_12 + off, h12 + off, (size_t)n * sizeof(double));
    if (chi2_21) std::memcpy(chi2_21 + off, h21 + off, (size_t)n * sizeof(double));
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_optimize_sim3_multi(int device, int n_problems, const int32_t* pair_off, const float* x3dc1, const float* x3dc2,
                                         const float* obs1, const float* obs2, const float* inv_sigma2_1, const float* inv_sigma2_2,
                                         const float* cam1, const float* cam2, const float* sim3_in, const float* th2,
                                         const uint8_t* fix_scale, double* sim3_out, uint8_t* bad, int32_t* n_in,
                                         orbfe_optsim3_stats* stats, double* chi2_12, double* chi2_21) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, "optimize_sim3_multi: negative device");
  if (const char* e = optsim3_check_multi(n_problems, pair_off, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2,
                                          sim3_in, th2, fix_scale, sim3_out, bad, n_in))
    return fail(ORBFE_ERR_INVALID, std::string("optimize_sim3_multi: ") + e);
  return run_multi(device, n_problems, pair_off, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, th2,
                   fix_scale, sim3_out, bad, n_in, stats, chi2_12, chi2_21);
}

extern "C" int orbfe_optimize_sim3(int device, int n, const float* x3dc1, const float* x3dc2, const float* obs1, const float* obs2,
                                   const float* inv_sigma2_1, const float* inv_sigma2_2, const float* cam1, const float* cam2,
                                   const float* sim3_in, float th2, int fix_scale, double* sim3_out, uint8_t* bad, int32_t* n_in,
                                   orbfe_optsim3_stats* stats, double* chi2_12, double* chi2_21) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, "optimize_sim3: negative device");
  if (const char* e = optsim3_check_single(n, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, th2,
                                           sim3_out, bad, n_in))
    return fail(ORBFE_ERR_INVALID, std::string("optimize_sim3: ") + e);
  const int32_t off[2] = {0, n};
  const uint8_t fix = fix_scale ? 1 : 0;
  return run_multi(device, 1, off, x3dc1, x3dc2, obs1, obs2, inv_sigma2_1, inv_sigma2_2, cam1, cam2, sim3_in, &th2, &fix, sim3_out,
                   bad, n_in, stats, chi2_12, chi2_21);
}
