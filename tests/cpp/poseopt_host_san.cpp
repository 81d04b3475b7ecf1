// Stand-alone program: the host side of orbfe_pose_optimization* (csrc/poseopt_host.h: argument checks and the interleaving
// of the edge arrays) on exactly-sized heap buffers, up to where the entry points would make their first device call.  Built with
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
  // the edge interleave: every source and destination array exactly as long as n says, every output element against its source
  for (int n : {0, 1, 15, 16, 17, 2049, kPoseOptHostMaxEdges}) {
    auto xw = exact<float>(3 * (size_t)n), u = exact<float>(n), v = exact<float>(n), ur = exact<float>(n), w = exact<float>(n);
    for (int i = 0; i < n; i++) {
      for (int k = 0; k < 3; k++) xw[3 * i + k] = (float)(3 * i + k) + 0.25f;
      u[i] = (float)i + 0.5f; v[i] = -(float)i - 1.0f; ur[i] = i % 2 ? -1.0f : (float)i - 0.125f; w[i] = 1.0f / (float)(i + 1);
    }
    auto A = exact<float>(4 * (size_t)n), B = exact<float>(4 * (size_t)n);
    for (size_t k = 0; k < 4 * (size_t)n; k++) A[k] = B[k] = -7.0f;  // (no packed value is -7)
    poseopt_pack_edges_a(A.get(), n, xw.get(), w.get());
    poseopt_pack_edges_b(B.get(), n, u.get(), v.get(), ur.get());
    for (int i = 0; i < n; i++) {
      EXPECT(A[4 * i] == xw[3 * i] && A[4 * i + 1] == xw[3 * i + 1] && A[4 * i + 2] == xw[3 * i + 2] && A[4 * i + 3] == w[i]);
      EXPECT(B[4 * i] == u[i] && B[4 * i + 1] == v[i] && B[4 * i + 2] == ur[i] && B[4 * i + 3] == 0.0f);
    }
  }
  std::printf("ok\n");
  return 0;
}
