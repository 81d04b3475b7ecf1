// orbfe_cpp::Optimizer::PoseOptimization (include/orbfe_classes.hpp) against the C-ABI on one mixed problem: the array form
// and the MapPointTable form.  Prints key=value tokens for tests/test_gpu_pose_opt_cpp.py.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbfe_classes.hpp"

int main() {
  using namespace orbfe_cpp;
  const int n = 300;
  const float K5[5] = {718.856f, 718.856f, 607.1928f, 185.2157f, 386.1448f};
  std::vector<float> Xw(3 * n), u(n), v(n), ur(n), w(n);
  std::vector<KeyPoint> keys(n);
  std::vector<float> invLevelSigma2(8);
  for (int l = 0; l < 8; l++) invLevelSigma2[l] = 1.0f / std::pow(1.2f, 2.0f * l);
  uint32_t s = 12345u;
  auto rnd = [&]() { s = s * 1664525u + 1013904223u; return (float)(s >> 8) / 16777216.0f; };
  for (int i = 0; i < n; i++) {  // points in front of an identity camera, a pixel of noise, every fifth edge a gross outlier
    const float z = 4.0f + 30.0f * rnd(), px = 30.0f + 1180.0f * rnd(), py = 20.0f + 330.0f * rnd();
    Xw[3 * i] = (px - K5[2]) / K5[0] * z; Xw[3 * i + 1] = (py - K5[3]) / K5[1] * z; Xw[3 * i + 2] = z;
    const float uu = K5[0] * Xw[3 * i] / z + K5[2], vv = K5[1] * Xw[3 * i + 1] / z + K5[3];
    u[i] = uu + (rnd() - 0.5f) + (i % 5 == 0 ? 60.0f : 0.0f);
    v[i] = vv + (rnd() - 0.5f);
    ur[i] = (i % 2) ? uu - K5[4] / z + (rnd() - 0.5f) : -1.0f;
    const int oct = i % 8;
    w[i] = invLevelSigma2[oct];
    keys[i] = KeyPoint{u[i], v[i], 31.0f, 0.0f, 1.0f, oct, -1};
  }
  float T0[16] = {1, 0, 0, 0.02f, 0, 1, 0, -0.03f, 0, 0, 1, 0.04f, 0, 0, 0, 1};

  // the C-ABI
  float Tc[16];
  std::vector<uint8_t> oc(n, 0);
  int32_t nc = 0;
  orbfe_poseopt_stats sc;
  std::memset(&sc, 0, sizeof sc);  // (the struct has padding: memcmp below)
  int rc = orbfe_pose_optimization(0, n, Xw.data(), u.data(), v.data(), ur.data(), w.data(), K5, T0, Tc, oc.data(), &nc, &sc, nullptr);
  if (rc != ORBFE_OK) { std::printf("error=%s\n", orbfe_last_error()); return 1; }

  // the class, array form
  float Ta[16];
  std::memcpy(Ta, T0, sizeof Ta);
  std::vector<uint8_t> oa;
  orbfe_poseopt_stats sa;
  std::memset(&sa, 0, sizeof sa);  // (the struct has padding: memcmp below)
  const int na = Optimizer::PoseOptimization(Xw, u, v, ur, w, K5, Ta, oa, &sa);

  // the class, table form: edge i in slot n - 1 - i, one extra keypoint on a bad slot
  MapPointTable table(n + 1);
  std::vector<int32_t> slot(n + 1), match(n + 1);
  std::vector<float> pos(3 * (n + 1)), normal(3 * (n + 1), 0.0f), lo(n + 1, 0.0f), hi(n + 1, 1.0f);
  std::vector<uint8_t> flags(n + 1, ORBFE_MP_OBSERVED), desc(32 * (size_t)(n + 1), 0);
  for (int i = 0; i <= n; i++) {
    slot[i] = n - i;
    match[i] = i;
    const int e = i < n ? i : 0;
    for (int k = 0; k < 3; k++) pos[3 * i + k] = Xw[3 * e + k];
  }
  flags[n] = ORBFE_MP_BAD;
  table.update(slot, pos, normal, lo, hi, desc, flags);
  std::vector<KeyPoint> keysT(keys);
  keysT.push_back(keys[0]);
  std::vector<float> urT(ur);
  urT.push_back(ur[0]);
  std::vector<uint8_t> descF(32 * (size_t)(n + 1), 0);
  FrameArrays F(keysT, descF, 0.0f, 1241.0f, 0.0f, 376.0f, urT);
  float Tt[16];
  std::memcpy(Tt, T0, sizeof Tt);
  std::vector<uint8_t> ot(n + 1, 5);
  orbfe_poseopt_stats st;
  std::memset(&st, 0, sizeof st);  // (the struct has padding: memcmp below)
  const int nt = Optimizer::PoseOptimization(table, slot, F, match, invLevelSigma2, K5, Tt, ot, &st);

  const bool arrayEq = na == nc && !std::memcmp(Ta, Tc, sizeof Tc) && oa == oc && !std::memcmp(&sa, &sc, sizeof sc);
  const bool tableEq = nt == nc && !std::memcmp(Tt, Tc, sizeof Tc) && std::equal(oc.begin(), oc.end(), ot.begin()) && ot[n] == 5 &&
                       !std::memcmp(&st, &sc, sizeof sc);
  int planted = 0, flagged = 0;
  for (int i = 0; i < n; i++) { planted += i % 5 == 0; flagged += oc[i] && i % 5 == 0; }
  std::printf("n=%d inliers=%d rounds=%d array_equal=%d table_equal=%d planted=%d planted_flagged=%d\n", n, nc, sc.rounds, (int)arrayEq,
              (int)tableEq, planted, flagged);
  return 0;
}
