// The loop-correction methods of include/orbfe_classes.hpp -- LoopClosing::CorrectedSim3s, MapPointTable::CorrectLoop,
// LoopClosing::PropagateGBA, MapPointTable::GlobalBundleAdjustmentUpdate -- on a world made by a formula that
// tests/test_gpu_loop_correct_cpp.py repeats: prints what the classes return, one "key=value" token per result (floats and
// doubles as their bit patterns), for the test to compare with the Python binding and the restatement.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

template <typename T>
static void print_ints(const char* key, const std::vector<T>& v) {
  std::printf("%s=", key);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%lld", i ? "," : "", (long long)v[i]);
  std::printf("\n");
}
static void print_bits(const char* key, const std::vector<float>& v) {
  std::vector<int64_t> b;
  for (float x : v) { uint32_t u; std::memcpy(&u, &x, 4); b.push_back((int64_t)u); }
  print_ints(key, b);
}
static void print_bits(const char* key, const std::vector<double>& v) {
  std::vector<int64_t> b;
  for (double x : v) { int64_t u; std::memcpy(&u, &x, 8); b.push_back(u); }
  print_ints(key, b);
}

// rotation number r (0 identity, 1 a quarter turn about z, 2 about x, 3 a half turn about y, 4 a quarter turn about y)
// with translation t, row-major 4 x 4
static void pose_of(int r, float tx, float ty, float tz, float* T) {
  static const float R[5][9] = {{1, 0, 0, 0, 1, 0, 0, 0, 1}, {0, -1, 0, 1, 0, 0, 0, 0, 1}, {1, 0, 0, 0, 0, -1, 0, 1, 0},
                                {-1, 0, 0, 0, 1, 0, 0, 0, -1}, {0, 0, 1, 0, 1, 0, -1, 0, 0}};
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) T[4 * i + j] = R[r][3 * i + j];
    T[4 * i + 3] = i == 0 ? tx : (i == 1 ? ty : tz);
  }
  T[12] = T[13] = T[14] = 0.f; T[15] = 1.f;
}
// the inverse of such a pose: exact, every entry is 0 or +-1 times a translation
static void inverse_of(const float* T, float* I) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) I[4 * i + j] = T[4 * j + i];
    I[4 * i + 3] = -(T[i] * T[3] + T[4 + i] * T[7] + T[8 + i] * T[11]);
  }
  I[12] = I[13] = I[14] = 0.f; I[15] = 1.f;
}

int main() {
  const int P = 200, CAP = 256, NKF = 7, W = 64;
  ObservationGraph g(CAP, 8, 8);
  MapPointTable mp(CAP);
  std::vector<int32_t> kfSlot, all, ref;
  std::vector<int64_t> mnId;
  std::vector<float> Ow;
  std::vector<uint8_t> bad;
  for (int k = 0; k < NKF; k++) {
    kfSlot.push_back(k); mnId.push_back(100 + 3 * k);
    Ow.push_back(0.5f * k); Ow.push_back(-0.25f * k); Ow.push_back(0.125f * k);
  }
  g.SetKeyFrames(kfSlot, mnId, Ow, std::vector<uint8_t>(NKF, 0));
  // observers (p % 7, (p + 3) % 7, (p + 5) % 7); the reference key frame is the first, or for every fifth point one outside the row
  std::vector<int32_t> oSlot, oKf;
  std::vector<uint16_t> oIdx;
  std::vector<uint8_t> oOct, oStereo;
  std::vector<float> pos, normal, lo, hi;
  for (int p = 0; p < P; p++) {
    all.push_back(p);
    bad.push_back(p % 17 == 5);
    ref.push_back(p % 5 == 0 ? (p + 1) % 7 : p % 7);
    for (int d : {0, 3, 5}) {
      oSlot.push_back(p); oKf.push_back((p + d) % 7); oIdx.push_back((uint16_t)p); oOct.push_back((uint8_t)((p + d) % 8)); oStereo.push_back(0);
    }
    pos.push_back((float)(p % 10) - 4.5f); pos.push_back((float)(p % 7) - 3.0f); pos.push_back(4.0f + (float)(p % 5));
    normal.push_back(0.f); normal.push_back(0.f); normal.push_back(1.f);
    lo.push_back(0.125f); hi.push_back(128.0f);
  }
  g.SetPoints(all, bad, ref);
  g.AddObservations(oSlot, oKf, oIdx, oOct, oStereo);
  mp.update(all, pos, normal, lo, hi, std::vector<uint8_t>(32 * P, 0), std::vector<uint8_t>(P, 0));
  int threw = 0;
  const std::vector<int32_t> order = {4, 1, 6, 0, 2};
  const int K = (int)order.size(), cur = 2;
  std::vector<float> Tiw(16 * K), TwcCur(16), OwNew, sf;
  for (int k = 0; k < K; k++) {
    pose_of(k, 0.5f * k, 0.25f, -0.125f * k, &Tiw[16 * k]);
    OwNew.push_back(0.5f * k + 0.25f); OwNew.push_back(1.0f); OwNew.push_back(-(float)k);
  }
  inverse_of(&Tiw[16 * cur], TwcCur.data());
  for (int i = 0; i < 8; i++) sf.push_back(1.0f + 0.25f * i);
  const std::vector<double> Scw = {0, 0, 0, 1, 0.5, -0.25, 0.125, 1.25};
  const LoopClosing::Sim3s S = LoopClosing::CorrectedSim3s(Tiw, TwcCur, cur, Scw);
  print_bits("corrected", S.corrected);
  print_bits("noncorrected", S.noncorrected);
  print_bits("tiw_corrected", S.TiwCorrected);
  try {
    LoopClosing::CorrectedSim3s(Tiw, TwcCur, K, Scw);  // cur outside [0, K)
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    mp.CorrectLoop(g, order, S.corrected, S.noncorrected, OwNew, sf);  // key-frame rows not enabled
  } catch (const std::runtime_error&) {
    threw++;
  }
  g.EnableKeyFramePoints(W);
  for (int k = 0; k < NKF; k++) {
    std::vector<int32_t> row;
    for (int i = 0; i < 40 + k; i++) row.push_back((i * 5 + k) % 4 == 0 ? -1 : (i * 7 + k * 31) % P);
    g.SetKeyFramePoints(k, row);
  }
  const MapPointTable::LoopCorrection c = mp.CorrectLoop(g, order, S.corrected, S.noncorrected, OwNew, sf, {3, 10});
  print_ints("slots", c.slots);
  print_ints("ref", c.ref);
  print_ints("valid", c.valid);
  print_bits("positions", mp.Positions(all));
  orbfe_camera_pose pose{};
  pose.Rcw[0] = pose.Rcw[4] = pose.Rcw[8] = 1.0f;
  pose.tcw[2] = 14.0f; pose.Ow[2] = -14.0f;
  pose.fx = pose.fy = 500.0f; pose.cx = 320.0f; pose.cy = 240.0f; pose.mbf = 40.0f;
  pose.min_x = 0.0f; pose.max_x = 640.0f; pose.min_y = 0.0f; pose.max_y = 480.0f;
  pose.log_scale_factor = 0.25f; pose.n_levels = 8;
  const MapPointTable::Projection pr = mp.ProjectInFrustum(all, pose, -2.0f);
  print_ints("in_view", pr.mbTrackInView);
  print_ints("level", pr.mnTrackScaleLevel);
  print_bits("view_cos", pr.mTrackViewCos);
  try {
    std::vector<double> worse = S.corrected;
    worse[8 + 7] = 0.0;  // a scale of 0
    mp.CorrectLoop(g, order, worse, S.noncorrected, OwNew, sf);
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    mp.CorrectLoop(g, {7}, {0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0, 1, 0, 0, 0, 1}, {0, 0, 0}, sf);  // kf slot 7 was never set
  } catch (const std::runtime_error&) {
    threw++;
  }

  // the global bundle adjustment: 0 (origin, GBA) -> 1 (GBA), 2 (new) -> 3 (new); 0 -> 4 (new) -> 5 (GBA); 6 under no origin
  const std::vector<int32_t> childOffsets = {0, 3, 3, 4, 4, 5, 5, 5}, child = {1, 2, 4, 3, 5};
  const std::vector<uint8_t> inGBA = {1, 1, 0, 0, 0, 1, 0};
  std::vector<float> Tcw(16 * NKF), Twc(16 * NKF), TcwGBA(16 * NKF);
  for (int k = 0; k < NKF; k++) {
    pose_of(k % 5, 0.25f * k, -0.5f, 0.125f * k, &Tcw[16 * k]);
    inverse_of(&Tcw[16 * k], &Twc[16 * k]);
    pose_of((k + 2) % 5, 0.25f * k + 0.125f, -0.25f, 0.5f * k, &TcwGBA[16 * k]);
  }
  const LoopClosing::Propagation pg = LoopClosing::PropagateGBA({0}, childOffsets, child, Tcw, Twc, inGBA, TcwGBA);
  print_bits("tcw_new", pg.TcwNew);
  print_ints("reached", pg.reached);
  print_ints("visited", pg.visited);
  try {
    LoopClosing::PropagateGBA({0}, childOffsets, {1, 2, 4, 0, 5}, Tcw, Twc, inGBA, TcwGBA);  // a cycle
  } catch (const std::runtime_error&) {
    threw++;
  }
  // the compact list leaves key frame 3 out; Twc_new is the inverse of the propagated pose
  const std::vector<int32_t> compact = {5, 0, 2, 6, 1, 4};
  std::vector<uint8_t> reached, pInGBA;
  std::vector<float> TcwBef, TwcNew(16 * compact.size()), posGBA;
  for (size_t j = 0; j < compact.size(); j++) {
    const int k = compact[j];
    reached.push_back(pg.reached[k]);
    TcwBef.insert(TcwBef.end(), &Tcw[16 * k], &Tcw[16 * k] + 16);
    inverse_of(&pg.TcwNew[16 * k], &TwcNew[16 * j]);
  }
  for (int p = 0; p < P; p++) {
    pInGBA.push_back(p % 3 == 0);
    posGBA.push_back(0.5f * (p % 9)); posGBA.push_back(-0.25f * (p % 11)); posGBA.push_back(3.0f + (p % 4));
  }
  print_ints("moved", mp.GlobalBundleAdjustmentUpdate(g, all, pInGBA, posGBA, compact, reached, TcwBef, TwcNew));
  print_bits("positions_gba", mp.Positions(all));
  try {
    std::vector<int32_t> twice = all;
    twice[1] = 0;
    mp.GlobalBundleAdjustmentUpdate(g, twice, pInGBA, posGBA, compact, reached, TcwBef, TwcNew);
  } catch (const std::runtime_error&) {
    threw++;
  }
  std::printf("threw=%d\n", threw);
  return 0;
}
