// orbfe_cpp::ObservationGraph and MapPointTable::UpdateNormalAndDepth (include/orbfe_classes.hpp) on a world made by a
// formula that tests/test_gpu_obsgraph_cpp.py repeats: prints what the class returns, one "key=value" token per result
// (floats as their bit patterns), for the test to compare with the Python binding.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbfe_classes.hpp"

using namespace orbfe_cpp;

static unsigned bits(float f) {
  unsigned u;
  std::memcpy(&u, &f, 4);
  return u;
}

template <typename T>
static void print_ints(const char* key, const std::vector<T>& v) {
  std::printf("%s=", key);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%lld", i ? "," : "", (long long)v[i]);
  std::printf("\n");
}

static void print_floats(const char* key, const std::vector<float>& v) {
  std::printf("%s=", key);
  for (size_t i = 0; i < v.size(); i++) std::printf("%s%08x", i ? "," : "", bits(v[i]));
  std::printf("\n");
}

int main() {
  const int K = 6, P = 40;
  ObservationGraph g(P, 70, 8);
  std::vector<int32_t> kfSlot;
  std::vector<int64_t> mnId;
  std::vector<float> Ow;
  for (int k = 0; k < K; k++) {
    kfSlot.push_back(k);
    mnId.push_back(10 + (5 - k) * 2);
    Ow.push_back(0.25f * k); Ow.push_back(-0.5f * k); Ow.push_back(0.125f * k);
  }
  g.SetKeyFrames(kfSlot, mnId, Ow, std::vector<uint8_t>(K, 0));
  std::vector<int32_t> slot, obsKf, ref, all;
  std::vector<uint16_t> idx;
  std::vector<uint8_t> octave, stereo, bad;
  std::vector<float> pos;
  for (int p = 0; p < P; p++) {
    int first = -1;
    for (int k = 0; k < K; k++) {
      if ((p * 7 + k * 3) % 5 >= 2) continue;
      if (first < 0) first = k;
      slot.push_back(p); obsKf.push_back(k); idx.push_back((uint16_t)p);
      octave.push_back((uint8_t)((p + k) % 4)); stereo.push_back((p + 2 * k) % 3 == 0);
    }
    all.push_back(p);
    ref.push_back(first);
    bad.push_back(p % 11 == 10);
    pos.push_back(0.125f * p - 2.0f); pos.push_back(0.25f * (p % 5)); pos.push_back(5.0f + 0.5f * (p % 7));
  }
  g.SetPoints(all, bad, ref);
  g.AddObservations(slot, obsKf, idx, octave, stereo);
  std::vector<float> sf(8, 1.0f);
  for (int i = 1; i < 8; i++) sf[(size_t)i] = sf[(size_t)i - 1] * 1.2f;

  const ObservationGraph::Votes v = g.VotesOf(all, 2);
  print_ints("votes_kf", v.kfSlot);
  print_ints("votes_w", v.weight);
  const ObservationGraph::Connections c = ObservationGraph::UpdateConnections(v, mnId);
  print_ints("ordered_id", c.orderedId);
  print_ints("ordered_w", c.orderedWeight);
  std::printf("parent=%lld\n", (long long)c.parentId);

  // culling counts of candidates 1 and 3 over their own observations
  std::vector<int32_t> cand = {1, 3}, off = {0}, fs, nMPs, nRed;
  std::vector<uint8_t> fo;
  for (int32_t k : cand) {
    for (size_t i = 0; i < slot.size(); i++)
      if (obsKf[i] == k) { fs.push_back(slot[i]); fo.push_back(octave[i]); }
    off.push_back((int32_t)fs.size());
  }
  g.CullingCounts(cand, off, fs, fo, nMPs, nRed);
  print_ints("n_mps", nMPs);
  print_ints("n_redundant", nRed);

  const ObservationGraph::NormalDepth nd = g.UpdateNormalAndDepth(all, pos, sf);
  print_ints("valid", nd.valid);
  print_floats("normal", nd.normal);
  print_floats("min", nd.minDist);
  print_floats("max", nd.maxDist);

  // the table form against the array form's results written by hand, seen through isInFrustum
  MapPointTable a(P), b(P);
  const std::vector<float> n0(3 * P, 0.0f), lo0(P, 0.1f), hi0(P, 100.0f);
  const std::vector<uint8_t> desc(32 * P, 0), fl(P, 0);
  a.update(all, pos, n0, lo0, hi0, desc, fl);
  std::vector<float> n1 = n0, lo1 = lo0, hi1 = hi0;
  for (int p = 0; p < P; p++) {
    if (!nd.valid[(size_t)p]) continue;
    for (int i = 0; i < 3; i++) n1[3 * (size_t)p + i] = nd.normal[3 * (size_t)p + i];
    lo1[(size_t)p] = nd.minDist[(size_t)p]; hi1[(size_t)p] = nd.maxDist[(size_t)p];
  }
  b.update(all, pos, n1, lo1, hi1, desc, fl);
  const std::vector<uint8_t> valid = a.UpdateNormalAndDepth(g, all, sf);
  orbfe_camera_pose pose{};
  pose.Rcw[0] = pose.Rcw[4] = pose.Rcw[8] = 1.0f;
  pose.fx = pose.fy = 500.0f; pose.cx = 320.0f; pose.cy = 240.0f; pose.mbf = 40.0f;
  pose.min_x = 0.0f; pose.max_x = 640.0f; pose.min_y = 0.0f; pose.max_y = 480.0f;
  pose.log_scale_factor = 0.18232156f; pose.n_levels = 8;
  const MapPointTable::Projection pa = a.ProjectInFrustum(all, pose, -2.0f), pb = b.ProjectInFrustum(all, pose, -2.0f);
  int inView = 0;
  for (uint8_t x : pa.mbTrackInView) inView += x;
  const bool same = valid == nd.valid && pa.mbTrackInView == pb.mbTrackInView && pa.mnTrackScaleLevel == pb.mnTrackScaleLevel &&
                    !std::memcmp(pa.mTrackViewCos.data(), pb.mTrackViewCos.data(), 4 * P) && !std::memcmp(pa.dist.data(), pb.dist.data(), 4 * P);
  std::printf("table_equal=%d\nin_view=%d\n", same ? 1 : 0, inView);

  // the mutations, then the votes again
  const std::vector<uint8_t> became = g.EraseObservations({0, 1, 2}, {0, 0, 0});
  print_ints("became_bad", became);
  print_ints("erased_kf_bad", g.EraseKeyFrame(4));
  const ObservationGraph::Votes v2 = g.VotesOf(all, -1);
  print_ints("votes2_kf", v2.kfSlot);
  print_ints("votes2_w", v2.weight);

  int threw = 0;
  try { g.SetPoints(all, bad, {}); } catch (const std::invalid_argument&) { threw++; }
  try { g.AddObservations({0}, {70}, {0}, {0}, {0}); } catch (const std::runtime_error&) { threw++; }
  try { g.VotesOf({P}); } catch (const std::runtime_error&) { threw++; }
  std::printf("threw=%d\n", threw);
  return 0;
}
