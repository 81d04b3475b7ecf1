// The descriptor methods of orbfe_cpp::ObservationGraph and orbfe_cpp::MapPointTable (include/orbfe_classes.hpp) on a world
// made by a formula that tests/test_gpu_obsdesc_cpp.py repeats: prints what the classes return, one "key=value" token per
// result, for the test to compare with the Python binding and the restatement.
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
  const int K = 24, P = 60, W = 64;
  ObservationGraph g(P, K, 128);
  MapPointTable table(P);
  int threw = 0;
  try {
    g.ComputeDistinctiveDescriptors({1});  // not enabled
  } catch (const std::runtime_error&) {
    threw++;
  }
  g.EnableKeyFrameDescriptors(W);
  std::vector<int32_t> kfSlot, all, ref;
  std::vector<int64_t> mnId;
  std::vector<uint8_t> bad;
  for (int k = 0; k < K; k++) {
    kfSlot.push_back(k);
    mnId.push_back(500 - 7 * k);  // descending with the kf slot
  }
  g.SetKeyFrames(kfSlot, mnId, std::vector<float>(3 * K, 0.f), std::vector<uint8_t>(K, 0));
  // key frame k holds 10 + k descriptors; byte b of row i is a formula of (k, i, b) with few distinct rows, so medians tie
  for (int k = 0; k < K; k++) {
    std::vector<uint8_t> d((size_t)(10 + k) * 32);
    for (int i = 0; i < 10 + k; i++)
      for (int b = 0; b < 32; b++) d[(size_t)i * 32 + b] = (uint8_t)(((i + k) % 3) * 85 + (b == (i * 7 + k) % 32 ? 1 : 0));
    g.SetKeyFrameDescriptors(k, d);
  }
  print_ints("kf5_desc", g.GetKeyFrameDescriptors(5));
  for (int p = 0; p < P - 10; p++) {  // the last 10 slots are never set
    all.push_back(p);
    bad.push_back(p % 11 == 4);
    ref.push_back(-1);
  }
  g.SetPoints(all, bad, ref);
  // point p is seen by 1 + p % 9 key frames, kf = (p + 5 j) % K at idx (p + j) % 10; point 7 has no row
  std::vector<int32_t> oSlot, oKf;
  std::vector<uint16_t> oIdx;
  std::vector<uint8_t> oOct, oStereo;
  for (int p = 0; p < P - 10; p++) {
    if (p == 7) continue;
    for (int j = 0; j < 1 + p % 9; j++) {
      oSlot.push_back(p); oKf.push_back((p + 5 * j) % K); oIdx.push_back((uint16_t)((p + j) % 10)); oOct.push_back(0); oStereo.push_back(0);
    }
  }
  g.AddObservations(oSlot, oKf, oIdx, oOct, oStereo);
  {  // key frames 3 and 12 are bad
    g.SetKeyFrames({3, 12}, {500 - 21, 500 - 84}, std::vector<float>(6, 0.f), {1, 1});
  }
  std::vector<int32_t> slots;
  for (int p = 0; p < P; p += 1) slots.push_back((p * 7) % P);  // every slot once, in no order
  const ObservationGraph::Distinctive r = g.ComputeDistinctiveDescriptors(slots);
  print_ints("kf", r.kfSlot);
  print_ints("idx", r.idx);
  print_ints("valid", r.valid);
  print_ints("desc", r.desc);
  // the table form: every slot holds its own number in every descriptor byte before the call
  std::vector<uint8_t> own((size_t)P * 32), flags((size_t)P, 0);
  std::vector<int32_t> every;
  for (int p = 0; p < P; p++) {
    every.push_back(p);
    for (int b = 0; b < 32; b++) own[(size_t)p * 32 + b] = (uint8_t)(200 + p % 50);
  }
  std::vector<float> pos((size_t)3 * P), one((size_t)P, 1.f);
  for (size_t i = 0; i < pos.size(); i++) pos[i] = 0.25f * (float)i;
  table.update(every, pos, pos, one, one, own, flags);
  std::vector<int32_t> wkf, widx;
  print_ints("table_valid", table.ComputeDistinctiveDescriptors(g, slots, &wkf, &widx));
  print_ints("table_kf", wkf);
  print_ints("table_idx", widx);
  print_ints("table_desc", table.Descriptors(every));
  std::printf("positions_kept=%d\n", table.Positions(every) == pos ? 1 : 0);
  print_ints("table_valid_no_winners", table.ComputeDistinctiveDescriptors(g, {0, 1, 2}));
  try {
    table.ComputeDistinctiveDescriptors(g, {1, 2, 1});  // a slot named twice
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    g.SetKeyFrameDescriptors(0, std::vector<uint8_t>((size_t)(W + 1) * 32, 0));  // more rows than the store is wide
  } catch (const std::runtime_error&) {
    threw++;
  }
  try {
    g.SetKeyFrameDescriptors(0, std::vector<uint8_t>(33, 0));
  } catch (const std::invalid_argument&) {
    threw++;
  }
  try {
    table.Descriptors({P});
  } catch (const std::runtime_error&) {
    threw++;
  }
  std::printf("threw=%d\n", threw);
  return 0;
}
