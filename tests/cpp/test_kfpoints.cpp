// The key-frame-row methods of orbfe_cpp::ObservationGraph (include/orbfe_classes.hpp) on a world made by a formula that
// tests/test_gpu_kfpoints_cpp.py repeats: prints what the class returns, one "key=value" token per result, for the test to
// compare with the Python binding and the restatement.
#include <cstdio>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

template <typename T>
static void print_ints(const char* key, const std::vector<T>& v) {
  std::printf("%s=", key);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%lld", i ? "," : "", (long long)v[i]);
  std::printf("\n");
}

int main() {
  const int K = 20, P = 300, W = 64;
  ObservationGraph g(P, K, 8);
  int threw = 0;
  try {
    g.SetKeyFramePoints(0, {1});  // not enabled
  } catch (const std::runtime_error&) {
    threw++;
  }
  std::vector<int32_t> kfSlot, all, ref;
  std::vector<int64_t> mnId;
  std::vector<uint8_t> bad;
  for (int k = 0; k < K; k++) {
    kfSlot.push_back(k);
    mnId.push_back(100 + 3 * k);
  }
  g.SetKeyFrames(kfSlot, mnId, std::vector<float>(3 * K, 0.f), std::vector<uint8_t>(K, 0));
  for (int p = 0; p < P - 20; p++) {  // the last 20 slots are never set
    all.push_back(p);
    bad.push_back(p % 13 == 5);
    ref.push_back(-1);
  }
  g.SetPoints(all, bad, ref);
  // three mono observations for every third point, a stereo one on top for every sixth: nObs 0, 3 or 5
  std::vector<int32_t> oSlot, oKf;
  std::vector<uint16_t> oIdx;
  std::vector<uint8_t> oOct, oStereo;
  for (int p = 0; p < P - 20; p += 3)
    for (int k = 0; k < (p % 6 == 0 ? 4 : 3); k++) {
      oSlot.push_back(p); oKf.push_back(k); oIdx.push_back((uint16_t)p); oOct.push_back(0); oStereo.push_back(k == 3);
    }
  g.AddObservations(oSlot, oKf, oIdx, oOct, oStereo);
  g.EnableKeyFramePoints(W);
  for (int k = 0; k < K; k++) {
    std::vector<int32_t> row;
    const int n = k == 6 ? 0 : (k == 7 ? W : 40 + k);
    for (int i = 0; i < n; i++) row.push_back((i * 5 + k) % 4 == 0 ? -1 : (i * 7 + k * 31) % P);
    g.SetKeyFramePoints(k, row);
  }
  // a point at the last place of the first 1024-entry block (k = 15, idx = 63) and again at the first of the next
  g.SetKeyFramePoints(15, std::vector<int32_t>(W, -1));
  g.AssignKeyFramePoints({15, 16, 2, 2}, {63, 0, 1, 2}, {299 - 20, 299 - 20, -1, 11});
  print_ints("row2", g.GetKeyFramePoints(2));
  print_ints("row15_device", g.GetKeyFramePoints(15, true));
  std::vector<int32_t> q;
  for (int k = 0; k < K; k++) q.push_back(k);
  print_ints("local", g.UpdateLocalPoints(q));
  print_ints("local_small_capacity", g.UpdateLocalPoints(q, 7));  // grows to the count and repeats
  const std::vector<std::vector<int32_t>> lists = g.KeyFramePointsUnion({0, 2, 2, 5}, {16, 15, 3, 3, 9});
  print_ints("union0", lists[0]);
  print_ints("union1", lists[1]);
  print_ints("union2", lists[2]);
  print_ints("tracked0", g.TrackedMapPoints(q, 0));
  print_ints("tracked3", g.TrackedMapPoints(q, 3));
  print_ints("tracked4", g.TrackedMapPoints(q, 4));
  try {
    g.AssignKeyFramePoints({6}, {0}, {1});  // row 6 has length 0
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    g.UpdateLocalPoints({K});
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    g.EnableKeyFramePoints(128);
  } catch (const std::runtime_error&) {
    threw++;
  }
  std::printf("threw=%d\n", threw);
  return 0;
}
