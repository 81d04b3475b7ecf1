// Stand-alone program: the host side of orbfe_local_bundle_adjustment* / orbfe_bundle_adjustment (csrc/lba_host.h: argument
// checks, the index arrays, the packing) on exactly-sized heap buffers, up to where the entry points would make their first
// device call.  Built with -fsanitize=address,undefined and run on the CPU (tests/test_lba_host_san.py); nothing of it is
// loaded into Python.  Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <memory>

#include "lba_host.h"

using namespace orbfe;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)
#define SAYS(expr, text)                                                 \
  do {                                                                   \
    const char* _m = (expr);                                             \
    if (!_m || std::strcmp(_m, text) != 0) { std::printf("FAILED %s:%d: %s gave %s\n", __FILE__, __LINE__, #expr, _m ? _m : "NULL"); return 1; } \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

// nLocal local + nFixed fixed poses, nPoints points, every pose sees every point: nPoses edges per point
struct World {
  int nLocal, nFixed, nPoints, nEdges;
  std::unique_ptr<float[]> Tcw, cam, xw, u, v, ur, w;
  std::unique_ptr<uint8_t[]> fixedFlags;
  std::unique_ptr<int32_t[]> ep, ept;
  World(int l, int f, int p) : nLocal(l), nFixed(f), nPoints(p), nEdges((l + f) * p) {
    const size_t nT = (size_t)(l + f);
    Tcw = exact<float>(16 * nT); cam = exact<float>(5 * nT); xw = exact<float>(3 * (size_t)p);
    u = exact<float>(nEdges); v = exact<float>(nEdges); ur = exact<float>(nEdges); w = exact<float>(nEdges);
    fixedFlags = exact<uint8_t>(l); ep = exact<int32_t>(nEdges); ept = exact<int32_t>(nEdges);
    for (size_t j = 0; j < nT; j++) {
      for (int k = 0; k < 4; k++) Tcw[16 * j + 5 * k] = 1.0f;
      Tcw[16 * j + 3] = -0.3f * (float)j;
      cam[5 * j] = 500.0f; cam[5 * j + 1] = 500.0f; cam[5 * j + 2] = 320.0f; cam[5 * j + 3] = 240.0f; cam[5 * j + 4] = 40.0f;
    }
    for (int i = 0; i < p; i++) { xw[3 * i] = 0.1f * (float)i; xw[3 * i + 1] = -0.05f * (float)i; xw[3 * i + 2] = 5.0f + (float)(i % 7); }
    for (int e = 0; e < nEdges; e++) {
      ept[e] = e / (int)nT; ep[e] = e % (int)nT;
      u[e] = 300.0f; v[e] = 200.0f; ur[e] = e % 2 ? -1.0f : 290.0f; w[e] = 1.0f;
    }
  }
  LbaProblem q(bool flags = false) const {
    return LbaProblem{nLocal, nFixed, Tcw.get(), flags ? fixedFlags.get() : nullptr, cam.get(), nPoints, xw.get(), nEdges, ep.get(), ept.get(),
                      u.get(), v.get(), ur.get(), w.get()};
  }
};

int main() {
  for (int nLocal : {1, 2, 7}) {
    for (int nFixed : {0, 2}) {
      for (int nPoints : {1, 2, 63, 64, 65}) {
        World W(nLocal, nFixed, nPoints);
        for (int flags = 0; flags < 2; flags++) {
          if (flags) W.fixedFlags[0] = 1;
          const LbaProblem q = W.q(flags != 0);
          EXPECT(lba_check(q, false) == nullptr);
          const size_t nT = (size_t)(nLocal + nFixed), nP = (size_t)nPoints, nE = (size_t)W.nEdges;
          const int nFree = lba_count_free(q), nFreeEdges = lba_count_free_edges(q), nBlocks = lba_count_blocks(nFree);
          EXPECT(nFree == nLocal - flags && nFreeEdges == nFree * nPoints);
          auto cam8 = exact<float>(8 * nT), obs = exact<float>(4 * nE);
          auto freeOf = exact<int32_t>(nT), ptOff = exact<int32_t>(nP + 1), poseOff = exact<int32_t>((size_t)nFree + 1);
          auto poseEdge = exact<int32_t>((size_t)nFreeEdges), edgeOf = exact<int32_t>((size_t)nFree * nP), blocks = exact<int32_t>(2 * (size_t)nBlocks);
          auto pose = exact<double>(8 * nT), pt = exact<double>(3 * nP);
          lba_pack_cam(cam8.get(), q); lba_pack_obs(obs.get(), q); lba_fill_free_of(freeOf.get(), q); lba_fill_pt_off(ptOff.get(), q);
          lba_fill_pose_off(poseOff.get(), q); lba_fill_pose_edge(poseEdge.get(), q); lba_fill_edge_of(edgeOf.get(), q);
          lba_fill_blocks(blocks.get(), nFree); lba_pack_poses(pose.get(), q); lba_pack_points(pt.get(), q);
          EXPECT(ptOff[0] == 0 && ptOff[nP] == W.nEdges && poseOff[nFree] == nFreeEdges);
          for (int f = 0; f < nFree; f++)
            for (int i = poseOff[f]; i < poseOff[f + 1]; i++) {
              const int e = poseEdge[i];
              EXPECT(freeOf[W.ep[e]] == f && edgeOf[(size_t)f * nP + W.ept[e]] == e);
              EXPECT(i == poseOff[f] || poseEdge[i - 1] < e);
            }
          for (int p = 0; p < nPoints; p++)
            for (int e = ptOff[p]; e < ptOff[p + 1]; e++) EXPECT(W.ept[e] == p);
          if (nBlocks) EXPECT(blocks[0] == 0 && blocks[2 * nBlocks - 1] == nFree - 1 && blocks[2 * nBlocks - 2] == nFree - 1);
          EXPECT(std::fabs(pose[3] - 1.0) < 1e-12 && pose[7] == 0.0);
          double T[16];
          lba_pose_to_Tcw(pose.get() + 8 * (nT - 1), T);
          EXPECT(std::fabs(T[3] - (double)W.Tcw[16 * (nT - 1) + 3]) < 1e-12 && T[15] == 1.0);
        }
      }
    }
  }
  // every refusal
  {
    World W(2, 1, 3);
    LbaProblem q = W.q();
    auto with = [&](auto&& change) { LbaProblem c = W.q(); change(c); return lba_check(c, false); };
    SAYS(with([](LbaProblem& c) { c.nLocal = 0; }), "n_local must be at least 1");
    SAYS(with([](LbaProblem& c) { c.nLocal = kLbaMaxLocal + 1; }), "more than 256 local key frames");
    SAYS(with([](LbaProblem& c) { c.nFixed = -1; }), "negative n_fixed");
    SAYS(with([](LbaProblem& c) { c.nFixed = kLbaMaxPoses; }), "more than 65536 key frames");
    SAYS(with([](LbaProblem& c) { c.nPoints = 0; }), "n_points must be at least 1");
    SAYS(with([](LbaProblem& c) { c.nPoints = kLbaMaxPoints + 1; }), "more than 4194304 points");
    SAYS(with([](LbaProblem& c) { c.nEdges = 0; }), "n_edges must be at least 1");
    SAYS(with([](LbaProblem& c) { c.nEdges = kLbaMaxEdges + 1; }), "more than 16777216 edges");
    SAYS(with([](LbaProblem& c) { c.Tcw = nullptr; }), "NULL per-pose array");
    SAYS(with([](LbaProblem& c) { c.cam = nullptr; }), "NULL per-pose array");
    SAYS(with([](LbaProblem& c) { c.xw = nullptr; }), "NULL xw");
    SAYS(with([](LbaProblem& c) { c.invSigma2 = nullptr; }), "NULL per-edge array");
    SAYS(with([](LbaProblem& c) { c.edgePose = nullptr; }), "NULL per-edge array");
    { LbaProblem c = q; c.xw = nullptr; EXPECT(lba_check(c, true) == nullptr); }
    W.ep[4] = 3; SAYS(lba_check(q, false), "edge_pose out of range"); W.ep[4] = -1; SAYS(lba_check(q, false), "edge_pose out of range"); W.ep[4] = 1;
    W.ept[8] = 3; SAYS(lba_check(q, false), "edge_point out of range"); W.ept[8] = 2;
    W.ept[3] = 0; W.ept[2] = 1; SAYS(lba_check(q, false), "edges must be grouped by point: edge_point descends"); W.ept[2] = 0; W.ept[3] = 1;
    W.Tcw[7] = INFINITY; SAYS(lba_check(q, false), "a pose or camera entry is not finite"); W.Tcw[7] = 0.0f;
    W.cam[14] = NAN; SAYS(lba_check(q, false), "a pose or camera entry is not finite"); W.cam[14] = 40.0f;
    W.xw[8] = NAN; SAYS(lba_check(q, false), "a point coordinate is not finite"); EXPECT(lba_check(q, true) == nullptr); W.xw[8] = 5.0f;
    W.ur[8] = -INFINITY; SAYS(lba_check(q, false), "an observation is not finite"); W.ur[8] = -1.0f;
    W.w[0] = NAN; SAYS(lba_check(q, false), "an observation is not finite"); W.w[0] = 1.0f;
    for (int e = 3; e < 6; e++) W.ept[e] = 2;  // point 1 loses its edges (and point 2 sees every pose twice)
    SAYS(lba_check(q, false), "a point without any edge");
    for (int e = 3; e < 6; e++) W.ept[e] = 1;
    for (int e = 0; e < 9; e += 3) W.ep[e] = 2;  // pose 0 loses its edges
    SAYS(lba_check(q, false), "a free pose without any edge");
    { LbaProblem c = W.q(true); W.fixedFlags[0] = 1; SAYS(lba_check(c, false), "two edges join the same pose and point"); W.fixedFlags[0] = 0; }
    for (int e = 0; e < 9; e += 3) W.ep[e] = 0;
    World D(2, 1, 2);
    D.ep[1] = 0;  // point 0: pose 0 twice; pose 1 keeps its edge to point 1
    SAYS(lba_check(D.q(), false), "two edges join the same pose and point");
  }
  std::printf("ok\n");
  return 0;
}
