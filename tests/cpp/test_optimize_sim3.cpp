// orbfe_cpp::Optimizer::OptimizeSim3 / OptimizeSim3Multi (include/orbfe_classes.hpp) against the C-ABI on one mixed problem:
// 80 pairs of which every fifth is a planted outlier, a start a few degrees and percent off the planted transform; the same
// call with 12 pairs of which 4 are planted (the early return); mismatched lengths.  Prints key=value tokens
// (tests/test_gpu_optimize_sim3_cpp.py).
#include <cmath>
#include <cstdio>
#include <vector>

#include "orbfe_classes.hpp"

namespace {

struct Rng {
  uint64_t s;
  double uni() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (double)(s >> 11) / 9007199254740992.0; }
  double sym(double a) { return (2.0 * uni() - 1.0) * a; }
};

void rot(const double w[3], double R[9]) {  // Rodrigues
  const double th = std::sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double a = th > 0 ? std::sin(th) / th : 1.0, b = th > 0 ? (1.0 - std::cos(th)) / (th * th) : 0.5;
  const double K[9] = {0, -w[2], w[1], w[2], 0, -w[0], -w[1], w[0], 0};
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) {
      double k2 = 0;
      for (int k = 0; k < 3; k++) k2 += K[3 * r + k] * K[3 * k + c];
      R[3 * r + c] = (r == c) + a * K[3 * r + c] + b * k2;
    }
}

struct Problem {
  std::vector<int32_t> idx1;
  std::vector<float> X1, X2, o1, o2, w1, w2;
  std::vector<uint8_t> planted;
  float rec[13];
  double S12[8];
};

const float kCam[4] = {718.856f, 718.856f, 607.1928f, 185.2157f};

Problem make(int n, int every, uint64_t seed) {
  Rng g{seed};
  Problem P;
  const double w[3] = {0.05, -0.08, 0.03}, t[3] = {0.2, -0.1, 0.3}, s = 1.1;
  double R[9];
  rot(w, R);
  for (int i = 0; i < n; i++) {
    const double z = 6 + 30 * g.uni(), x2[3] = {(150 + 900 * g.uni() - kCam[2]) / kCam[0] * z, (60 + 250 * g.uni() - kCam[3]) / kCam[1] * z, z};
    double x1[3];
    for (int r = 0; r < 3; r++) x1[r] = s * (R[3 * r] * x2[0] + R[3 * r + 1] * x2[1] + R[3 * r + 2] * x2[2]) + t[r];
    const bool out = every > 0 && i % every == 2;
    P.idx1.push_back(3 * i + 1);
    for (int r = 0; r < 3; r++) { P.X1.push_back((float)x1[r]); P.X2.push_back((float)x2[r]); }
    P.o1.push_back((float)(kCam[0] * x1[0] / x1[2] + kCam[2] + g.sym(0.5) + (out ? 70.0 : 0.0)));
    P.o1.push_back((float)(kCam[1] * x1[1] / x1[2] + kCam[3] + g.sym(0.5)));
    P.o2.push_back((float)(kCam[0] * x2[0] / x2[2] + kCam[2] + g.sym(0.5)));
    P.o2.push_back((float)(kCam[1] * x2[1] / x2[2] + kCam[3] + g.sym(0.5) - (out ? 55.0 : 0.0)));
    P.w1.push_back(1.0f); P.w2.push_back(i % 2 ? 1.0f : 0.6944444f);
    P.planted.push_back(out ? 1 : 0);
  }
  const double dw[3] = {w[0] + 0.02, w[1] - 0.015, w[2] + 0.01};
  double Rs[9];
  rot(dw, Rs);
  for (int k = 0; k < 9; k++) P.rec[k] = (float)Rs[k];
  P.rec[9] = (float)(t[0] + 0.04); P.rec[10] = (float)(t[1] - 0.03); P.rec[11] = (float)(t[2] + 0.05); P.rec[12] = (float)(s * 1.03);
  // the start as g2o::Sim3 members: the quaternion of the float matrix (trace > 0 here)
  const double tr = std::sqrt((double)P.rec[0] + (double)P.rec[4] + (double)P.rec[8] + 1.0);
  P.S12[3] = 0.5 * tr;
  P.S12[0] = ((double)P.rec[7] - (double)P.rec[5]) * (0.5 / tr);
  P.S12[1] = ((double)P.rec[2] - (double)P.rec[6]) * (0.5 / tr);
  P.S12[2] = ((double)P.rec[3] - (double)P.rec[1]) * (0.5 / tr);
  for (int k = 0; k < 4; k++) P.S12[4 + k] = (double)P.rec[9 + k];
  return P;
}

}  // namespace

int main() {
  using orbfe_cpp::Optimizer;
  // the class against the C-ABI fed with the record the class derives
  Problem P = make(80, 5, 3);
  float rec[13];
  Optimizer::sim3_record(P.S12, rec);
  const int n = (int)P.idx1.size();
  std::vector<uint8_t> bad((size_t)n);
  double out[8];
  int32_t nIn = 0;
  orbfe_optsim3_stats st, stc;
  if (orbfe_optimize_sim3(0, n, P.X1.data(), P.X2.data(), P.o1.data(), P.o2.data(), P.w1.data(), P.w2.data(), kCam, kCam, rec, 10.0f, 0, out,
                          bad.data(), &nIn, &st, nullptr, nullptr) != 0) { std::printf("cabi_failed=1 %s\n", orbfe_last_error()); return 1; }
  std::vector<int32_t> vp(3 * (size_t)n + 5);
  for (size_t i = 0; i < vp.size(); i++) vp[i] = (int32_t)i + 1000;
  double S[8];
  for (int k = 0; k < 8; k++) S[k] = P.S12[k];
  const int got = Optimizer::OptimizeSim3(P.idx1, P.X1, P.X2, P.o1, P.o2, P.w1, P.w2, kCam, kCam, vp, S, 10.0f, false, &stc);
  int equal = got == nIn && stc.rounds == st.rounds && stc.n_bad == st.n_bad, erasedRight = 1, plantedErased = 0, planted = 0;
  for (int k = 0; k < 8; k++) equal = equal && S[k] == out[k];
  std::vector<uint8_t> hit(vp.size(), 0);
  for (int i = 0; i < n; i++) if (bad[i]) hit[(size_t)P.idx1[i]] = 1;
  for (size_t i = 0; i < vp.size(); i++) erasedRight = erasedRight && (hit[i] ? vp[i] == -1 : vp[i] == (int32_t)i + 1000);
  for (int i = 0; i < n; i++) { planted += P.planted[i]; plantedErased += P.planted[i] && bad[i]; }
  double moved = 0;
  for (int k = 0; k < 8; k++) moved = std::fmax(moved, std::fabs(S[k] - P.S12[k]));
  std::printf("rounds=%d n_in=%d class_equal=%d erased_right=%d planted=%d planted_erased=%d moved=%d\n", st.rounds, (int)nIn, equal,
              erasedRight, planted, plantedErased, moved > 1e-3);

  // the early return: 12 pairs of which 4 are planted; S12 stays, the erasures happen
  Problem E = make(12, 3, 5);
  std::vector<int32_t> vpe(3 * 12 + 5, 7);
  double Se[8];
  for (int k = 0; k < 8; k++) Se[k] = E.S12[k];
  orbfe_optsim3_stats ste;
  const int early = Optimizer::OptimizeSim3(E.idx1, E.X1, E.X2, E.o1, E.o2, E.w1, E.w2, kCam, kCam, vpe, Se, 10.0f, false, &ste);
  int untouched = 1, erasedE = 0;
  for (int k = 0; k < 8; k++) untouched = untouched && Se[k] == E.S12[k];
  for (int32_t v : vpe) erasedE += v == -1;
  std::printf("early_return=%d early_rounds=%d early_untouched=%d early_erased=%d early_n_bad=%d\n", early, ste.rounds, untouched, erasedE,
              ste.n_bad);

  // the multi form: both problems in one launch equal the single calls
  std::vector<int32_t> off = {0, n, n + 12}, idx = P.idx1;
  std::vector<float> X1 = P.X1, X2 = P.X2, o1 = P.o1, o2 = P.o2, w1 = P.w1, w2 = P.w2, K(kCam, kCam + 4);
  idx.insert(idx.end(), E.idx1.begin(), E.idx1.end());
  X1.insert(X1.end(), E.X1.begin(), E.X1.end()); X2.insert(X2.end(), E.X2.begin(), E.X2.end());
  o1.insert(o1.end(), E.o1.begin(), E.o1.end()); o2.insert(o2.end(), E.o2.begin(), E.o2.end());
  w1.insert(w1.end(), E.w1.begin(), E.w1.end()); w2.insert(w2.end(), E.w2.begin(), E.w2.end());
  K.insert(K.end(), kCam, kCam + 4);
  std::vector<std::vector<int32_t>> vpm(2);
  vpm[0].resize(vp.size());
  for (size_t i = 0; i < vp.size(); i++) vpm[0][i] = (int32_t)i + 1000;
  vpm[1].assign(vpe.size(), 7);
  std::vector<double> Sm(P.S12, P.S12 + 8);
  Sm.insert(Sm.end(), E.S12, E.S12 + 8);
  const std::vector<int> nin = Optimizer::OptimizeSim3Multi(off, idx, X1, X2, o1, o2, w1, w2, K, K, vpm, Sm, {10.0f, 10.0f}, {0, 0});
  int multiEqual = nin[0] == got && nin[1] == early && vpm[0] == vp && vpm[1] == vpe;
  for (int k = 0; k < 8; k++) multiEqual = multiEqual && Sm[k] == S[k] && Sm[8 + k] == Se[k];
  std::printf("multi_equal=%d\n", multiEqual);

  int threw = 0;
  try {
    std::vector<float> shortX(P.X1.begin(), P.X1.end() - 1);
    Optimizer::OptimizeSim3(P.idx1, shortX, P.X2, P.o1, P.o2, P.w1, P.w2, kCam, kCam, vp, S, 10.0f, false);
  } catch (const std::invalid_argument&) { threw++; }
  try {
    std::vector<int32_t> small(5, 0);
    Optimizer::OptimizeSim3(P.idx1, P.X1, P.X2, P.o1, P.o2, P.w1, P.w2, kCam, kCam, small, S, 10.0f, false);
  } catch (const std::invalid_argument&) { threw++; }
  try {
    Optimizer::OptimizeSim3Multi(off, idx, X1, X2, o1, o2, w1, w2, K, K, vpm, Sm, {10.0f}, {0, 0});
  } catch (const std::invalid_argument&) { threw++; }
  std::printf("threw=%d\n", threw);
  return 0;
}
