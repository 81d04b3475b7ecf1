// Stand-alone program: the host side of orbfe_triangulate_matches* (csrc/triangulate_host.h: argument checks, the pair list,
// the outputs of a call without pairs) and the per-pair arithmetic (csrc/triangulate_math.h) on exactly-sized heap buffers, up
// to where the entry points would make their first device call.  Built with -fsanitize=address,undefined and run on the CPU
// (tests/test_triangulate_host_san.py); nothing of it is loaded into Python.  Prints "ok" and returns 0.
#include <cstdio>
#include <memory>
#include <vector>

#include "triangulate_host.h"

using namespace orbfe;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

struct Frame {
  std::unique_ptr<float[]> x, y, ur, depth;
  std::unique_ptr<int32_t[]> oct;
  orbfe_frame_view v = {};
  orbfe_keyframe_camera c = {};
  Frame(int n, int levels, float shift) : x(exact<float>(n)), y(exact<float>(n)), ur(exact<float>(n)), depth(exact<float>(n)), oct(exact<int32_t>(n)) {
    for (int i = 0; i < n; i++) {
      x[i] = 100.0f + 3.0f * (float)(i % 97) + shift; y[i] = 80.0f + 2.0f * (float)(i % 89);
      ur[i] = i % 2 ? x[i] - 20.0f : -1.0f;
      depth[i] = i % 2 ? 5.0f : -1.0f;
      oct[i] = i % levels;
    }
    v.n = n; v.x = x.get(); v.y = y.get(); v.octave = oct.get(); v.u_right = ur.get();
    const float T[12] = {1, 0, 0, -shift / 100.0f, 0, 1, 0, 0, 0, 0, 1, 0};
    memcpy(c.Tcw, T, sizeof T);
    c.Ow[0] = shift / 100.0f;
    c.fx = c.fy = 500.0f; c.cx = 320.0f; c.cy = 240.0f; c.invfx = c.invfy = 1.0f / 500.0f; c.mb = 0.2f; c.mbf = 100.0f;
    c.depth = depth.get();
  }
};

int main() {
  const int L = 8;
  auto sf = exact<float>(L), sg = exact<float>(L);
  for (int l = 0; l < L; l++) { sf[l] = 1.0f + 0.2f * (float)l; sg[l] = sf[l] * sf[l]; }
  for (int K : {0, 1, 3, kTriHostMaxNeighbours})
    for (int n1 : {0, 1, 65, 257}) {
      Frame f1(n1, L, 0.0f);
      std::vector<std::unique_ptr<Frame>> nb;
      std::vector<const orbfe_frame_view*> views;
      auto cams = exact<orbfe_keyframe_camera>(K);
      for (int k = 0; k < K; k++) {
        nb.emplace_back(new Frame(n1 + k % 3, L, 40.0f + (float)k));
        views.push_back(&nb[k]->v);
        cams[k] = nb[k]->c;
      }
      const size_t slots = (size_t)K * n1;
      auto match = exact<int32_t>(slots);
      for (size_t s = 0; s < slots; s++) match[s] = s % 3 == 0 ? -1 : (int32_t)((s * 7) % (size_t)(n1 + (int)(s / n1) % 3));
      auto x3d = exact<float>(slots * 3);
      auto status = exact<uint8_t>(slots);
      auto created = exact<int32_t>(K), winner = exact<int32_t>(n1);
      const orbfe_frame_view* const* vv = K ? views.data() : nullptr;
      auto ok = [&]() { return triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(),
                                                 status.get(), created.get(), winner.get(), true); };
      EXPECT(ok() == nullptr);
      std::vector<TriangulatePair> pairs;
      triangulate_pairs(&f1.v, &f1.c, K, vv, cams.get(), match.get(), &pairs);
      triangulate_init_outputs(K, n1, x3d.get(), status.get(), created.get(), winner.get());
      size_t live = 0;
      for (size_t s = 0; s < slots; s++) live += match[s] >= 0;
      EXPECT(pairs.size() == live);
      for (const TriangulatePair& p : pairs) {  // the arithmetic, as the kernel's lane runs it
        EXPECT(p.k >= 0 && p.k < K && p.i1 >= 0 && p.i1 < n1 && p.i2 >= 0 && p.i2 < views[p.k]->n);
        const Frame& g = *nb[p.k];
        const TriKeypoint k1 = {f1.x[p.i1], f1.y[p.i1], f1.ur[p.i1], p.depth1, p.xraw1, p.yraw1, sg[f1.oct[p.i1]], sf[f1.oct[p.i1]]};
        const TriKeypoint k2 = {g.x[p.i2], g.y[p.i2], g.ur[p.i2], p.depth2, p.xraw2, p.yraw2, sg[g.oct[p.i2]], sf[g.oct[p.i2]]};
        double X[3] = {0, 0, 0};
        const int st = tri_pair(tri_camera(&f1.c), tri_camera(&cams[p.k]), k1, k2, 1.8f, X);
        EXPECT(st >= kTriCreated && st <= kTriScale);
        const size_t slot = (size_t)p.k * n1 + p.i1;
        status[slot] = (uint8_t)st;
        x3d[3 * slot + 2] = (float)X[2];
      }
      // every refusal
      EXPECT(triangulate_check(nullptr, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, nullptr, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), nullptr, sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), nullptr, L, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), 0, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), ORBFE_MAX_LEVELS + 1, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, &f1.c, -1, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
      EXPECT(triangulate_check(&f1.v, &f1.c, kTriHostMaxNeighbours + 1, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
      if (n1 > 0) {
        EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), nullptr, true));
        EXPECT((triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), nullptr, false) == nullptr));
        orbfe_frame_view broken = f1.v;
        broken.octave = nullptr;
        EXPECT(triangulate_check(&broken, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
        broken = f1.v; broken.n = kTriHostMaxKeypoints + 1;
        EXPECT(triangulate_check(&broken, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
      }
      if (K > 0) {
        EXPECT(triangulate_check(&f1.v, &f1.c, K, nullptr, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
        EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, nullptr, match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
        EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), nullptr, winner.get(), true));
        const orbfe_frame_view* keep = views[K - 1];
        views[K - 1] = nullptr; EXPECT(ok()); views[K - 1] = keep;
      }
      if (K > 0 && n1 > 1) {
        EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), nullptr, sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
        EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, nullptr, status.get(), created.get(), winner.get(), true));
        EXPECT(triangulate_check(&f1.v, &f1.c, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), nullptr, created.get(), winner.get(), true));
        const size_t last = slots - 1;  // slot (K - 1, n1 - 1)
        const int32_t keep = match[last];
        const int n2 = views[K - 1]->n;
        match[last] = n2; EXPECT(ok()); match[last] = -2; EXPECT(ok());
        match[last] = n2 - 1; EXPECT(ok() == nullptr);
        Frame& g = *nb[K - 1];
        g.oct[n2 - 1] = L; EXPECT(ok()); g.oct[n2 - 1] = -1; EXPECT(ok()); g.oct[n2 - 1] = 0;
        f1.oct[n1 - 1] = L; EXPECT(ok()); f1.oct[n1 - 1] = 0;
        // a matched stereo keypoint needs a positive depth
        g.ur[n2 - 1] = 5.0f; g.depth[n2 - 1] = 0.0f; EXPECT(ok()); g.depth[n2 - 1] = 2.0f; EXPECT(ok() == nullptr);
        cams[K - 1].depth = nullptr; EXPECT(ok()); cams[K - 1].depth = g.depth.get();
        f1.ur[n1 - 1] = 5.0f; f1.depth[n1 - 1] = 1.0f;
        orbfe_keyframe_camera nodepth = f1.c; nodepth.depth = nullptr;
        EXPECT(triangulate_check(&f1.v, &nodepth, K, vv, cams.get(), match.get(), sf.get(), sg.get(), L, x3d.get(), status.get(), created.get(), winner.get(), true));
        match[last] = -1;
        f1.oct[n1 - 1] = 99; EXPECT(K > 1 || ok() == nullptr);  // (an unmatched keypoint's octave is not read)
        f1.oct[n1 - 1] = 0;
        match[last] = keep;
      }
    }
  std::printf("ok\n");
  return 0;
}
