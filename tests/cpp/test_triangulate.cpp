// orbfe_cpp::ORBmatcher::TriangulateMatchesMulti / TriangulateMatches (include/orbfe_classes.hpp) on one scene file written by
// tests/test_gpu_triangulate_cpp.py (tests/triangulate_ref.py: write_scene): writes status / x3d / n_created / winner of the
// multi form for the Python test to compare, and prints whether host views, resident frames and the single form agree.
#include <cstdio>
#include <memory>
#include <vector>

#include "orbfe_classes.hpp"
#include "triangulate_scene.h"

int main(int argc, char** argv) {
  using namespace orbfe_cpp;
  if (argc < 3) return 2;
  TriScene S;
  if (!tri_read_scene(argv[1], &S)) { std::printf("error=cannot_read_scene\n"); return 2; }
  std::vector<std::unique_ptr<FrameArrays>> frames;
  std::vector<std::unique_ptr<KeyFrameCamera>> cams;
  for (const TriSceneFrame& F : S.frames) {
    std::vector<KeyPoint> keys((size_t)F.n);
    for (int i = 0; i < F.n; i++) keys[i] = KeyPoint{F.x[i], F.y[i], 31.0f, 0.0f, 1.0f, F.octave[i], -1};
    frames.emplace_back(new FrameArrays(keys, std::vector<uint8_t>(32 * (size_t)F.n, 0), 0.0f, 640.0f, 0.0f, 480.0f,
                                        F.stereo ? F.ur : std::vector<float>()));
    cams.emplace_back(new KeyFrameCamera(F.cam.Tcw, F.cam.Ow, F.cam.fx, F.cam.fy, F.cam.cx, F.cam.cy, F.cam.invfx, F.cam.invfy,
                                         F.cam.mb, F.cam.mbf, F.stereo ? F.depth : std::vector<float>(),
                                         F.raw ? F.xraw : std::vector<float>(), F.raw ? F.yraw : std::vector<float>()));
  }
  std::vector<const FrameArrays*> nb;
  std::vector<const KeyFrameCamera*> nc;
  for (int k = 0; k < S.K; k++) { nb.push_back(frames[1 + k].get()); nc.push_back(cams[1 + k].get()); }
  ORBmatcher matcher(0.6f, false);
  std::vector<float> x3d, x3dR, xs;
  std::vector<uint8_t> status, statusR, ss;
  std::vector<int32_t> created, createdR, winner, winnerR;
  try {
    matcher.TriangulateMatchesMulti(*frames[0], *cams[0], nb, nc, S.match12, S.scaleFactors, S.levelSigma2, S.ratioFactor, x3d,
                                    status, created, winner);
    bool singleEq = true;
    for (int k = 0; k < S.K; k++) {
      const std::vector<int32_t> m(S.match12.begin() + (size_t)k * S.n1, S.match12.begin() + (size_t)(k + 1) * S.n1);
      const int n = matcher.TriangulateMatches(*frames[0], *cams[0], *nb[k], *nc[k], m, S.scaleFactors, S.levelSigma2,
                                               S.ratioFactor, xs, ss);
      singleEq = singleEq && n == created[k] && !std::memcmp(xs.data(), x3d.data() + (size_t)k * S.n1 * 3, xs.size() * 4) &&
                 !std::memcmp(ss.data(), status.data() + (size_t)k * S.n1, ss.size());
    }
    for (auto& f : frames) f->makeResident();
    matcher.TriangulateMatchesMulti(*frames[0], *cams[0], nb, nc, S.match12, S.scaleFactors, S.levelSigma2, S.ratioFactor, x3dR,
                                    statusR, createdR, winnerR);
    const bool residentEq = x3dR.size() == x3d.size() && !std::memcmp(x3dR.data(), x3d.data(), x3d.size() * 4) &&
                            statusR == status && createdR == created && winnerR == winner;
    std::vector<int32_t> rest(created);
    rest.insert(rest.end(), winner.begin(), winner.end());
    if (!tri_write_result(argv[2], status, x3d, rest)) return 2;
    std::printf("single_equal=%d resident_equal=%d\n", (int)singleEq, (int)residentEq);
  } catch (const std::exception& e) {
    std::printf("error=%s\n", e.what());
    return 1;
  }
  return 0;
}
