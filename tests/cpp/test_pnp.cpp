// orbfe_cpp::PnPsolver (include/orbfe_classes.hpp) on one scene file written by tests/test_gpu_pnp_cpp.py (tests/pnp_ref.py:
// write_scene with sigma2 in the sixth column): the multi-candidate form PnPsolver::make_all with
// SetRansacParameters(0.99, 10, 300, 4, 0.5, 5.991) as src/Tracking.cc:1494, then the caller's round-robin of iterate(5)
// (:1503-1560) until every solver has returned a pose or said bNoMore.  Prints one line per call.
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <vector>

#include "orbfe_classes.hpp"

int main(int argc, char** argv) {
  if (argc < 2) { std::printf("error=usage\n"); return 2; }
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("error=cannot_read_scene\n"); return 2; }
  int K = 0;
  if (std::fscanf(f, "%d", &K) != 1 || K < 0) return 2;
  std::vector<int32_t> pointOff(1, 0), kp, nKp;
  std::vector<float> p3d, p2d, sigma2, cam;
  std::vector<std::vector<int32_t>> sets((size_t)K);
  for (int k = 0; k < K; k++) {
    int n, H, mi;
    float c[4];
    if (std::fscanf(f, "%d %d %d %f %f %f %f", &n, &H, &mi, c, c + 1, c + 2, c + 3) != 7) return 2;
    cam.insert(cam.end(), c, c + 4);
    for (int i = 0; i < n; i++) {
      float v[6];
      if (std::fscanf(f, "%f %f %f %f %f %f", v, v + 1, v + 2, v + 3, v + 4, v + 5) != 6) return 2;
      p3d.insert(p3d.end(), v, v + 3); p2d.insert(p2d.end(), v + 3, v + 5); sigma2.push_back(v[5]);
      kp.push_back(2 * i + 1);  // mvKeyPointIndices: every other key point
    }
    nKp.push_back(2 * n + 3);
    sets[(size_t)k].resize(4 * (size_t)H);
    for (int i = 0; i < 4 * H; i++)
      if (std::fscanf(f, "%d", &sets[(size_t)k][(size_t)i]) != 1) return 2;
    pointOff.push_back(pointOff.back() + n);
  }
  std::fclose(f);
  try {
    {  // before solve_all
      orbfe_cpp::PnPsolver lone(std::vector<float>(p3d.begin(), p3d.begin() + 3 * pointOff[1]),
                                std::vector<float>(p2d.begin(), p2d.begin() + 2 * pointOff[1]),
                                std::vector<float>(sigma2.begin(), sigma2.begin() + pointOff[1]),
                                std::vector<int32_t>(kp.begin(), kp.begin() + pointOff[1]), cam.data(), nKp[0]);
      lone.SetRansacParameters(0.99, 4, 300, 4, 0.1f, 5.991f);
      bool nm; std::vector<bool> vb; int ni; float T[16];
      int threw = 0;
      try { lone.iterate(5, nm, vb, ni, T); } catch (const std::logic_error&) { threw = 1; }
      std::printf("iterate_before_solve_throws %d\n", threw);
    }
    std::vector<orbfe_cpp::PnPsolver> solvers =
        orbfe_cpp::PnPsolver::make_all(pointOff, p3d, p2d, sigma2, kp, cam, nKp, sets, 0.99, 10, 300, 4, 0.5f, 5.991f);
    for (int k = 0; k < K; k++)
      std::printf("solver %d %d %d %d\n", k, solvers[(size_t)k].N(), solvers[(size_t)k].minInliers(), solvers[(size_t)k].maxIterations());
    std::vector<int> done((size_t)K, 0);
    int left = K;
    while (left > 0) {
      for (int k = 0; k < K; k++) {
        if (done[(size_t)k]) continue;
        bool bNoMore = false;
        std::vector<bool> vb;
        int nInliers = 0;
        float T[16];
        int found = 0, ran_out = 0;
        try {
          found = solvers[(size_t)k].iterate(5, bNoMore, vb, nInliers, T) ? 1 : 0;
        } catch (const std::out_of_range&) { ran_out = 1; }
        long cnt = 0, sum = 0;
        for (size_t i = 0; i < vb.size(); i++)
          if (vb[i]) { cnt++; sum += (long)i; }
        std::printf("call %d %d %d %d %d %ld %ld %d %zu", k, ran_out, found, bNoMore ? 1 : 0, nInliers, cnt, sum,
                    solvers[(size_t)k].iterations(), vb.size());
        if (found)
          for (int i = 0; i < 3; i++) std::printf(" %.9g %.9g %.9g %.9g", T[4 * i], T[4 * i + 1], T[4 * i + 2], T[4 * i + 3]);
        std::printf("\n");
        if (found || bNoMore || ran_out) { done[(size_t)k] = 1; left--; }
      }
    }
  } catch (const std::exception& e) {
    std::printf("error=%s\n", e.what());
    return 1;
  }
  return 0;
}
