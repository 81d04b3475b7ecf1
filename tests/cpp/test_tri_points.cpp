// The triangulated-point methods of include/orbfe_classes.hpp -- ORBmatcher::TriangulatedPointsSelect and
// MapPointTable::CreateTriangulatedPoints -- on one scene file written by tests/test_gpu_tri_points_cpp.py
// (tests/triangulate_ref.py: write_scene), with descriptors made by a formula the test repeats: prints what the classes
// return, one "key=value" token per result (floats as their bit patterns), for the test to compare with the Python binding.
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "orbfe_classes.hpp"
#include "triangulate_scene.h"

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

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  TriScene S;
  if (!tri_read_scene(argv[1], &S)) { std::printf("error=cannot_read_scene\n"); return 2; }
  const int K = S.K, n1 = S.n1, CAP = 2 * n1 + 8;
  const std::vector<int32_t> kfSlots = {1, 3, 0, 4};
  const std::vector<int64_t> kfIds = {10, 3, 30, 11};
  if (K > 3) return 2;
  std::vector<std::unique_ptr<FrameArrays>> frames;
  std::vector<std::unique_ptr<KeyFrameCamera>> cams;
  std::vector<float> centres;
  int widest = 0;
  for (size_t j = 0; j < S.frames.size(); j++) {
    const TriSceneFrame& F = S.frames[j];
    std::vector<KeyPoint> keys((size_t)F.n);
    std::vector<uint8_t> desc(32 * (size_t)F.n);
    for (int i = 0; i < F.n; i++) {
      keys[(size_t)i] = KeyPoint{F.x[(size_t)i], F.y[(size_t)i], 31.0f, 0.0f, 1.0f, F.octave[(size_t)i], -1};
      for (int b = 0; b < 32; b++) desc[(size_t)i * 32 + b] = (uint8_t)((i * 131 + b * 17 + (int)j * 7) % 256);
    }
    frames.emplace_back(new FrameArrays(keys, desc, 0.0f, 640.0f, 0.0f, 480.0f, F.stereo ? F.ur : std::vector<float>()));
    frames.back()->makeResident();
    cams.emplace_back(new KeyFrameCamera(F.cam.Tcw, F.cam.Ow, F.cam.fx, F.cam.fy, F.cam.cx, F.cam.cy, F.cam.invfx, F.cam.invfy,
                                         F.cam.mb, F.cam.mbf, F.stereo ? F.depth : std::vector<float>(),
                                         F.raw ? F.xraw : std::vector<float>(), F.raw ? F.yraw : std::vector<float>()));
    for (int r = 0; r < 3; r++) centres.push_back(F.cam.Ow[r]);
    widest = F.n > widest ? F.n : widest;
  }
  std::vector<const FrameArrays*> nb;
  std::vector<const KeyFrameCamera*> nc;
  for (int k = 0; k < K; k++) { nb.push_back(frames[1 + (size_t)k].get()); nc.push_back(cams[1 + (size_t)k].get()); }
  const std::vector<int32_t> slots(kfSlots.begin(), kfSlots.begin() + 1 + K), nbSlots(kfSlots.begin() + 1, kfSlots.begin() + 1 + K);
  const std::vector<int64_t> ids(kfIds.begin(), kfIds.begin() + 1 + K), nbIds(kfIds.begin() + 1, kfIds.begin() + 1 + K);
  try {
    ORBmatcher matcher(0.6f, false);
    std::vector<float> x3d;
    std::vector<uint8_t> status;
    std::vector<int32_t> created, winner;
    matcher.TriangulateMatchesMulti(*frames[0], *cams[0], nb, nc, S.match12, S.scaleFactors, S.levelSigma2, S.ratioFactor, x3d, status,
                                    created, winner);
    const std::vector<float> c1(centres.begin(), centres.begin() + 3), c2(centres.begin() + 3, centres.end());
    const ORBmatcher::TriangulatedPoints sel = ORBmatcher::TriangulatedPointsSelect(n1, S.match12, status, x3d, ids[0], nbIds, c1, c2,
                                                                                    frames[0]->octave, S.scaleFactors, n1);
    print_ints("sel_k", sel.k); print_ints("sel_i1", sel.i1); print_ints("sel_i2", sel.i2); print_ints("sel_from", sel.descFrom);
    print_bits("sel_pos", sel.pos); print_bits("sel_normal", sel.normal); print_bits("sel_min", sel.minDist); print_bits("sel_max", sel.maxDist);

    ObservationGraph g(CAP, 6, 8);
    MapPointTable mp(CAP);
    g.SetKeyFrames(slots, ids, centres, std::vector<uint8_t>(slots.size(), 0));
    g.EnableKeyFramePoints((widest + 63) / 64 * 64);
    for (size_t j = 0; j < slots.size(); j++) g.SetKeyFramePoints(slots[j], std::vector<int32_t>((size_t)S.frames[j].n, -1));
    std::vector<int32_t> newSlot;
    for (int j = 0; j < n1; j++) newSlot.push_back(CAP - 1 - 2 * j);
    const MapPointTable::CreatedTriangulatedPoints made = mp.CreateTriangulatedPoints(g, *frames[0], slots[0], *cams[0], nb, nbSlots, nc, S.match12,
                                                                                      S.scaleFactors, S.levelSigma2, S.ratioFactor, newSlot);
    print_ints("k", made.k); print_ints("i1", made.i1); print_ints("i2", made.i2); print_ints("slot", made.slot);
    print_ints("status", made.status); print_ints("per_neighbour", made.perNeighbour);
    print_bits("positions", mp.Positions(made.slot));
    print_ints("descriptors", mp.Descriptors(made.slot));
    print_ints("kf1_row", g.GetKeyFramePoints(slots[0]));

    int threw = 0;
    auto refused = [&](int kf1Slot, const std::vector<int32_t>& kf2, const std::vector<int32_t>& free) {
      try {
        MapPointTable t(CAP);
        t.CreateTriangulatedPoints(g, *frames[0], kf1Slot, *cams[0], nb, kf2, nc, S.match12, S.scaleFactors, S.levelSigma2, S.ratioFactor, free);
      } catch (const std::exception&) { threw++; }
    };
    std::vector<int32_t> fresh;
    for (int j = 0; j < n1; j++) fresh.push_back(CAP - 2 - 2 * j);
    refused(2, nbSlots, fresh);                        // a kf slot never set
    refused(nbSlots[0], nbSlots, fresh);               // key frame 1 is one of the neighbours
    refused(slots[0], nbSlots, newSlot);               // the slots' rows are live by now
    refused(slots[0], nbSlots, {fresh[0], fresh[1]});  // more points than slots: capacity
    refused(slots[0], nbSlots, {fresh[0], fresh[1], fresh[0]});  // a slot named twice
    std::printf("threw=%d\n", threw);
  } catch (const std::exception& e) {
    std::printf("error=%s\n", e.what());
    return 1;
  }
  return 0;
}
