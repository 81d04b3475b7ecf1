// Stand-alone program: the per-pair arithmetic of csrc/triangulate_math.h -- the very code k_triangulate.hip compiles for the
// device -- and the pair list of csrc/triangulate_host.h on the CPU.  Reads a scene file (tests/triangulate_ref.py:
// write_scene), writes status / x3d / n_created / winner, prints the single-thread time of the pair loop.  Build with
// -ffp-contract=off (tests/test_triangulate_math_cpu.py).
#include <chrono>
#include <cstdlib>
#include <cstdio>
#include <vector>

#include "triangulate_host.h"
#include "triangulate_scene.h"

using namespace orbfe;

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: triangulate_cpu scene result [repeats]\n"); return 2; }
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 1;
  TriScene S;
  if (!tri_read_scene(argv[1], &S)) { std::printf("cannot read %s\n", argv[1]); return 2; }
  const int K = S.K, n1 = S.n1;
  const size_t slots = (size_t)K * n1;
  std::vector<float> x3d(slots * 3 + 1);
  std::vector<uint8_t> status(slots + 1);
  std::vector<int32_t> nCreated((size_t)K + 1), winner((size_t)n1 + 1);
  const orbfe_frame_view* f1 = &S.frames[0].view;
  const orbfe_keyframe_camera* cam1 = &S.frames[0].cam;
  if (const char* e = triangulate_check(f1, cam1, K, S.views2.data(), S.cams2.data(), S.match12.data(), S.scaleFactors.data(),
                                        S.levelSigma2.data(), S.nLevels, x3d.data(), status.data(), nCreated.data(), winner.data(), true)) {
    std::printf("refused: %s\n", e);
    return 1;
  }
  std::vector<TriangulatePair> pairs;
  std::vector<TriCamera> cams;
  double bestUs = 1e300;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    triangulate_pairs(f1, cam1, K, S.views2.data(), S.cams2.data(), S.match12.data(), &pairs);
    triangulate_init_outputs(K, n1, x3d.data(), status.data(), nCreated.data(), winner.data());
    cams.clear();
    cams.push_back(tri_camera(cam1));
    for (int k = 0; k < K; k++) cams.push_back(tri_camera(&S.cams2[k]));
    for (const TriangulatePair& p : pairs) {
      const orbfe_frame_view* g = S.views2[p.k];
      const int o1 = f1->octave[p.i1], o2 = g->octave[p.i2];
      const TriKeypoint k1 = {f1->x[p.i1], f1->y[p.i1], f1->u_right ? f1->u_right[p.i1] : -1.0f, p.depth1, p.xraw1, p.yraw1,
                              S.levelSigma2[o1], S.scaleFactors[o1]};
      const TriKeypoint k2 = {g->x[p.i2], g->y[p.i2], g->u_right ? g->u_right[p.i2] : -1.0f, p.depth2, p.xraw2, p.yraw2,
                              S.levelSigma2[o2], S.scaleFactors[o2]};
      double X[3] = {0.0, 0.0, 0.0};
      const int st = tri_pair(cams[0], cams[1 + p.k], k1, k2, S.ratioFactor, X);
      const size_t slot = (size_t)p.k * n1 + p.i1;
      status[slot] = (uint8_t)st;
      if (st == kTriCreated) {
        x3d[3 * slot] = (float)X[0]; x3d[3 * slot + 1] = (float)X[1]; x3d[3 * slot + 2] = (float)X[2];
        nCreated[p.k]++;
        if (winner[p.i1] < 0 || p.k < winner[p.i1]) winner[p.i1] = p.k;
      }
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < bestUs) bestUs = us;
  }
  status.resize(slots); x3d.resize(slots * 3);
  std::vector<int32_t> rest(nCreated.begin(), nCreated.begin() + K);
  rest.insert(rest.end(), winner.begin(), winner.begin() + n1);
  if (!tri_write_result(argv[2], status, x3d, rest)) return 2;
  std::printf("pairs=%zu cpu_us=%.1f\n", pairs.size(), bestUs);
  return 0;
}
