// Stand-alone program: the host side of orbfe_pose_optimization* (csrc/poseopt_host.h: argument checks and the arena layout)
// on exactly-sized heap buffers, up to where the entry points would make their first device call.  Built with
// -fsanitize=address,undefined and run on the CPU (tests/test_poseopt_host_san.py); nothing of it is loaded into Python.
// Prints "ok" and returns 0.
#include <cstdio>
#include <memory>

#include "poseopt_host.h"

using namespace orbfe;

#define EXPECT(cond)                                                     \
  do {                                                                   \
    if (!(cond)) { std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

template <typename T>
static std::unique_ptr<T[]> exact(size_t n) { return std::unique_ptr<T[]>(new T[n ? n : 1]()); }

int main() {
  // single form: every array exactly as long as the call says
  for (int n : {0, 1, 2, 3, 9, 10, 257, 2048, 2049, kPoseOptHostMaxEdges}) {
    auto xw = exact<float>(3 * (size_t)n), u = exact<float>(n), v = exact<float>(n), ur = exact<float>(n), w = exact<float>(n);
    auto K5 = exact<float>(5), Tin = exact<float>(16), Tout = exact<float>(16);
    auto fl = exact<uint8_t>(n);
    int32_t ni = 0;
    EXPECT(poseopt_check_single(n, xw.get(), u.get(), v.get(), ur.get(), w.get(), K5.get(), Tin.get(), Tout.get(), fl.get(), &ni) == nullptr);
    EXPECT(poseopt_check_single(n, xw.get(), u.get(), v.get(), ur.get(), w.get(), nullptr, Tin.get(), Tout.get(), fl.get(), &ni));
    EXPECT(poseopt_check_single(n, xw.get(), u.get(), v.get(), ur.get(), w.get(), K5.get(), Tin.get(), Tout.get(), fl.get(), nullptr));
    if (n > 0) {
      EXPECT(poseopt_check_single(n, nullptr, u.get(), v.get(), ur.get(), w.get(), K5.get(), Tin.get(), Tout.get(), fl.get(), &ni));
      EXPECT(poseopt_check_single(n, xw.get(), u.get(), v.get(), ur.get(), w.get(), K5.get(), Tin.get(), Tout.get(), nullptr, &ni));
    }
  }
  {
    float k[5] = {}, t[16] = {}, o[16] = {};
    int32_t ni = 0;
    EXPECT(poseopt_check_single(-1, nullptr, nullptr, nullptr, nullptr, nullptr, k, t, o, nullptr, &ni));
    EXPECT(poseopt_check_single(kPoseOptHostMaxEdges + 1, nullptr, nullptr, nullptr, nullptr, nullptr, k, t, o, nullptr, &ni));
  }
  // batch form: Q + 1 offsets, read only up to the first defect
  for (int Q : {0, 1, 3, 512}) {
    auto off = exact<int32_t>((size_t)Q + 1);
    for (int p = 0; p <= Q; p++) off[p] = 7 * p;
    const int N = 7 * Q;
    auto xw = exact<float>(3 * (size_t)N), a = exact<float>(N), K5 = exact<float>(5 * (size_t)Q), T = exact<float>(16 * (size_t)Q);
    auto fl = exact<uint8_t>(N);
    auto ni = exact<int32_t>(Q);
    EXPECT(poseopt_check_batch(Q, off.get(), xw.get(), a.get(), a.get(), a.get(), a.get(), K5.get(), T.get(), T.get(), fl.get(), ni.get()) == nullptr);
    EXPECT(poseopt_check_batch(Q, nullptr, xw.get(), a.get(), a.get(), a.get(), a.get(), K5.get(), T.get(), T.get(), fl.get(), ni.get()));
    if (Q >= 3) {
      off[2] = off[1] - 1;  // descends
      EXPECT(poseopt_check_batch(Q, off.get(), xw.get(), a.get(), a.get(), a.get(), a.get(), K5.get(), T.get(), T.get(), fl.get(), ni.get()));
      off[2] = off[1] + kPoseOptHostMaxEdges + 1;  // one problem too large
      EXPECT(poseopt_check_batch(Q, off.get(), xw.get(), a.get(), a.get(), a.get(), a.get(), K5.get(), T.get(), T.get(), fl.get(), ni.get()));
    }
    off[0] = 1;
    EXPECT(poseopt_check_batch(Q, off.get(), xw.get(), a.get(), a.get(), a.get(), a.get(), K5.get(), T.get(), T.get(), fl.get(), ni.get()));
  }
  {
    int32_t off[1] = {0};
    EXPECT(poseopt_check_batch(-1, off, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
    EXPECT(poseopt_check_batch(kPoseOptHostMaxProblems + 1, off, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr));
  }
  // table form
  {
    const int cap = 50, ns = 40, nf = 30, nl = 8;
    auto slot = exact<int32_t>(ns), match = exact<int32_t>(nf), oct = exact<int32_t>(nf);
    auto x = exact<float>(nf), lv = exact<float>(nl), K5 = exact<float>(5), T = exact<float>(16);
    auto fl = exact<uint8_t>(nf);
    int32_t ni = 0;
    for (int i = 0; i < ns; i++) slot[i] = cap - 1 - i;
    for (int i = 0; i < nf; i++) { match[i] = i % 3 ? i : -1; oct[i] = i % nl; }
    auto ok = [&]() { return poseopt_check_table(cap, ns, slot.get(), nf, match.get(), oct.get(), x.get(), x.get(), lv.get(), nl, K5.get(), T.get(), T.get(), fl.get(), &ni); };
    EXPECT(ok() == nullptr);
    slot[ns - 1] = cap; EXPECT(ok()); slot[ns - 1] = -1; EXPECT(ok()); slot[ns - 1] = 0;
    match[nf - 1] = ns; EXPECT(ok()); match[nf - 1] = ns - 1; EXPECT(ok() == nullptr);
    oct[nf - 1] = nl; EXPECT(ok()); oct[nf - 1] = -1; EXPECT(ok()); oct[nf - 1] = 0;
    oct[0] = 99; EXPECT(ok() == nullptr);  // (feature 0 has no match: its octave is not read)
    EXPECT(poseopt_check_table(cap, ns, slot.get(), kPoseOptHostMaxEdges + 1, match.get(), oct.get(), x.get(), x.get(), lv.get(), nl, K5.get(), T.get(), T.get(), fl.get(), &ni));
    EXPECT(poseopt_check_table(cap, ns, slot.get(), nf, match.get(), oct.get(), x.get(), x.get(), lv.get(), 0, K5.get(), T.get(), T.get(), fl.get(), &ni));
  }
  // layout: ascending, aligned, every array inside the total
  for (int table = 0; table < 2; table++)
    for (int N : {0, 1, 255, 2049, kPoseOptHostMaxEdges})
      for (int Q : {1, 512}) {
        if (table && Q != 1) continue;
        const PoseOptLayout L = poseopt_layout(Q, N, table != 0, true, 1000, 8, 96, 152);
        const size_t n = (size_t)(N ? N : 1);
        EXPECT(L.upEnd <= L.downBegin && L.downBegin == L.oRes && L.total % 256 == 0 && L.upEnd % 256 == 0);
        EXPECT(L.oEdgeA + n * 16 <= L.oEdgeB && L.oRes + (size_t)Q * 152 <= L.oLevel && L.oLevel + n <= L.oChi2 && L.oChi2 + n * 8 <= L.total);
        if (table) EXPECT(L.oSlot + 4000 <= L.oMatch && L.oFeatOct + n * 4 <= L.oLevelTab && L.oLevelTab + 32 <= L.upEnd &&
                          L.oEdgeA >= L.upEnd && L.oEdgeB + n * 16 <= L.downBegin && L.oEdgeFeat + n * 4 <= L.total);
        else EXPECT(L.oEdgeB + n * 16 <= L.upEnd);
      }
  std::printf("ok\n");
  return 0;
}
