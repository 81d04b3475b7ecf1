// triangulate.hip -- C-ABI entry points of the triangulation of CreateNewMapPoints' matched pairs (include/orbfe.h,
// "LocalMapping::CreateNewMapPoints").  A call is one staged copy up, ONE launch of k_triangulate (k_triangulate.hip) and one
// copy back on the calling thread's matcher stream, complete on return.  The argument checks and the pair list are
// triangulate_host.h (no device needed).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "arena.h"
#include "frame.h"
#include "host_internal.h"
#include "triangulate_host.h"
#include "triangulate_kernels.h"

using namespace orbfe;

namespace {

// a frame's keypoint arrays for the kernel: a resident frame's own, else uploaded with the call
hipError_t stage_frame(Arena* a, const orbfe_frame_view* given, const orbfe_frame_view* host, TriangulateFrame* out) {
  TriangulateFrame f = {};
  if (const orbfe_frame* R = given->resident) {
    f.x = R->dx; f.y = R->dy; f.octave = R->doct; f.ur = host->u_right ? R->dur : nullptr;
  } else {
    const size_t n = (size_t)host->n;
    float *dx, *dy, *dur = nullptr;
    int32_t* doct;
    TRY(up(a, &dx, host->x, n)); TRY(up(a, &dy, host->y, n)); TRY(up(a, &doct, host->octave, n));
    if (host->u_right) TRY(up(a, &dur, host->u_right, n));
    f.x = dx; f.y = dy; f.octave = doct; f.ur = dur;
  }
  *out = f;
  return hipSuccess;
}

int run(const char* who, int device, const orbfe_frame_view* KF1, const orbfe_keyframe_camera* cam1, int K,
        const orbfe_frame_view* const* KF2, const orbfe_keyframe_camera* cam2, const int32_t* match12,
        const float* scale_factors, const float* level_sigma2, int n_levels, float ratio_factor, float* x3d, uint8_t* status,
        int32_t* n_created, int32_t* winner, bool wantWinner) {
  if (device < 0) return fail(ORBFE_ERR_INVALID, std::string(who) + ": negative device");
  if (!KF1 || (K > 0 && !KF2)) return fail(ORBFE_ERR_INVALID, std::string(who) + ": NULL key frame");
  if (K < 0 || K > kTriHostMaxNeighbours) return fail(ORBFE_ERR_INVALID, std::string(who) + ": n_neighbours outside [0, 64]");
  const orbfe_frame_view* h1 = canon(KF1);
  std::vector<const orbfe_frame_view*> h2((size_t)K);
  for (int k = 0; k < K; k++) h2[k] = canon(KF2[k]);
  if (const char* e = triangulate_check(h1, cam1, K, h2.data(), cam2, match12, scale_factors, level_sigma2, n_levels, x3d, status,
                                        n_created, winner, wantWinner))
    return fail(ORBFE_ERR_INVALID, std::string(who) + ": " + e);
  if (KF1->resident && KF1->resident->device != device) return fail(ORBFE_ERR_INVALID, std::string(who) + ": key frame 1 is resident on another device");
  for (int k = 0; k < K; k++)
    if (KF2[k]->resident && KF2[k]->resident->device != device)
      return fail(ORBFE_ERR_INVALID, std::string(who) + ": a neighbour is resident on another device");
  const int n1 = h1->n;
  std::vector<TriangulatePair> pairs;
  triangulate_pairs(h1, cam1, K, h2.data(), cam2, match12, &pairs);
  triangulate_init_outputs(K, n1, x3d, status, n_created, winner);
  if (pairs.empty()) return ORBFE_OK;

  UnsettledScope unsettledScope;
  std::vector<TriCamera> cams((size_t)K + 1);
  cams[0] = tri_camera(cam1);
  for (int k = 0; k < K; k++) cams[1 + k] = tri_camera(cam2 + k);
  std::vector<TriangulateFrame> frames((size_t)K + 1);
  const size_t slots = (size_t)K * (size_t)n1;
  TriangulateArgs A = {};
  Arena* ar;
  auto stage = [&](Arena* a) -> hipError_t {
    TriangulatePair* dpairs;
    TriCamera* dcams;
    float *dsf, *dsg;
    TRY(stage_frame(a, KF1, h1, &frames[0]));
    for (int k = 0; k < K; k++) TRY(stage_frame(a, KF2[k], h2[k], &frames[1 + k]));
    TRY(up(a, &dpairs, pairs.data(), pairs.size()));
    TRY(up(a, &dcams, cams.data(), cams.size()));
    TRY(up(a, &dsf, scale_factors, (size_t)n_levels));
    TRY(up(a, &dsg, level_sigma2, (size_t)n_levels));
    TriangulateFrame* dframes = carve<TriangulateFrame>(a, frames.size());  // (device addresses: known once the frames are carved)
    TRY(put(a, dframes, frames.data(), frames.size()));
    open_span(a);  // the four outputs adjacent: one copy back
    TRY(up_fill(a, &A.x3d, slots * 3, 0));
    TRY(up_fill(a, &A.status, slots, 0));
    TRY(up_fill(a, &A.nCreated, (size_t)K, 0));
    TRY(up_fill(a, &A.winner, (size_t)n1, 0x7f));
    TRY(close_span(a));
    A.pairs = dpairs; A.nPairs = (int)pairs.size(); A.n1 = n1;
    A.frames = dframes; A.cams = dcams; A.scaleFactors = dsf; A.levelSigma2 = dsg; A.ratioFactor = ratio_factor;
    return hipSuccess;
  };
  HIPCHK(arena_stage(device, &ar, stage));
  HIPCHK(frame_use(ar, KF1->resident));
  for (int k = 0; k < K; k++) HIPCHK(frame_use(ar, KF2[k]->resident));
  HIPCHK(flush(ar));
  launch_triangulate(ar->stream, A);
  HIPCHK(hipGetLastError());
  HIPCHK(down_span(ar));
  HIPCHK(hipStreamSynchronize(ar->stream));
  frames_settle();
  std::memcpy(x3d, mirror_of(ar, A.x3d), slots * 3 * sizeof(float));
  std::memcpy(status, mirror_of(ar, A.status), slots);
  std::memcpy(n_created, mirror_of(ar, A.nCreated), (size_t)K * 4);
  if (winner) {
    const int32_t* w = mirror_of(ar, A.winner);
    for (int i = 0; i < n1; i++) winner[i] = w[i] == kTriangulateNoWinner ? -1 : w[i];
  }
  return ORBFE_OK;
}

}  // namespace

extern "C" int orbfe_triangulate_matches_multi(int device, const orbfe_frame_view* KF1, const orbfe_keyframe_camera* cam1,
                                               int n_neighbours, const orbfe_frame_view* const* KF2,
                                               const orbfe_keyframe_camera* cam2, const int32_t* match12,
                                               const float* scale_factors, const float* level_sigma2, int n_levels,
                                               float ratio_factor, float* x3d, uint8_t* status, int32_t* n_created,
                                               int32_t* winner) {
  return run("triangulate_matches_multi", device, KF1, cam1, n_neighbours, KF2, cam2, match12, scale_factors, level_sigma2,
             n_levels, ratio_factor, x3d, status, n_created, winner, true);
}

extern "C" int orbfe_triangulate_matches(int device, const orbfe_frame_view* KF1, const orbfe_keyframe_camera* cam1,
                                         const orbfe_frame_view* KF2, const orbfe_keyframe_camera* cam2, const int32_t* match12,
                                         const float* scale_factors, const float* level_sigma2, int n_levels, float ratio_factor,
                                         float* x3d, uint8_t* status, int32_t* n_created) {
  if (!KF2) return fail(ORBFE_ERR_INVALID, "triangulate_matches: NULL key frame");
  return run("triangulate_matches", device, KF1, cam1, 1, &KF2, cam2, match12, scale_factors, level_sigma2, n_levels,
             ratio_factor, x3d, status, n_created, nullptr, false);
}
