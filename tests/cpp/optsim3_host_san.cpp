// Stand-alone program: the host side of orbfe_optimize_sim3* (csrc/optsim3_host.h: argument checks and the packing of the
// pair and problem records) on exactly-sized heap buffers, up to where the entry points would make their first device call.
// Built with -fsanitize=address,undefined and run on the CPU (tests/test_optsim3_host_san.py); nothing of it is loaded into
// Python.  Prints "ok" and returns 0.
#include <cmath>
#include <cstdio>
#include <cstring>
#include <limits>
#include <memory>

#include "optsim3_host.h"

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

int main() {
  // single form: every array exactly as long as the call says
  for (int n : {0, 1, 9, 10, 15, 16, 17, 31, 32, 33, 255, 256, 257, kOptSim3HostMaxPairs}) {
    auto x1 = exact<float>(3 * (size_t)n), x2 = exact<float>(3 * (size_t)n), o1 = exact<float>(2 * (size_t)n), o2 = exact<float>(2 * (size_t)n);
    auto w1 = exact<float>(n), w2 = exact<float>(n), c1 = exact<float>(4), c2 = exact<float>(4), s = exact<float>(13);
    auto out = exact<double>(8);
    auto bad = exact<uint8_t>(n);
    int32_t ni = 0;
    auto chk = [&](const float* a, const float* cam, const uint8_t* b, const int32_t* pn, float th2) {
      return optsim3_check_single(n, a, x2.get(), o1.get(), o2.get(), w1.get(), w2.get(), cam, c2.get(), s.get(), th2, out.get(), b, pn);
    };
    EXPECT(chk(x1.get(), c1.get(), bad.get(), &ni, 10.0f) == nullptr);
    SAYS(chk(x1.get(), nullptr, bad.get(), &ni, 10.0f), "NULL per-problem array");
    SAYS(chk(x1.get(), c1.get(), bad.get(), nullptr, 10.0f), "NULL per-problem array");
    SAYS(chk(x1.get(), c1.get(), bad.get(), &ni, 0.0f), "th2 must be positive and finite");
    SAYS(chk(x1.get(), c1.get(), bad.get(), &ni, -1.0f), "th2 must be positive and finite");
    SAYS(chk(x1.get(), c1.get(), bad.get(), &ni, std::numeric_limits<float>::infinity()), "th2 must be positive and finite");
    SAYS(chk(x1.get(), c1.get(), bad.get(), &ni, std::nanf("")), "th2 must be positive and finite");
    if (n > 0) {
      SAYS(chk(nullptr, c1.get(), bad.get(), &ni, 10.0f), "NULL per-pair array");
      SAYS(chk(x1.get(), c1.get(), nullptr, &ni, 10.0f), "NULL per-pair array");
    }
  }
  {
    float c[4] = {}, s[13] = {};
    double out[8];
    int32_t ni = 0;
    SAYS(optsim3_check_single(-1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c, c, s, 10.0f, out, nullptr, &ni), "negative count");
    SAYS(optsim3_check_single(kOptSim3HostMaxPairs + 1, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, c, c, s, 10.0f, out, nullptr, &ni),
         "more than 16384 pairs");
  }
  // multi form: K + 1 offsets, read only up to the first defect
  for (int K : {0, 1, 3, 512}) {
    auto off = exact<int32_t>((size_t)K + 1);
    for (int p = 0; p <= K; p++) off[p] = 7 * p;
    const int N = 7 * K;
    auto x = exact<float>(3 * (size_t)N), o = exact<float>(2 * (size_t)N), w = exact<float>(N);
    auto cam = exact<float>(4 * (size_t)K), s = exact<float>(13 * (size_t)K), th2 = exact<float>(K);
    auto fix = exact<uint8_t>(K), bad = exact<uint8_t>(N);
    auto out = exact<double>(8 * (size_t)K);
    auto ni = exact<int32_t>(K);
    for (int p = 0; p < K; p++) th2[p] = 10.0f;
    auto chk = [&](const int32_t* po) {
      return optsim3_check_multi(K, po, x.get(), x.get(), o.get(), o.get(), w.get(), w.get(), cam.get(), cam.get(), s.get(), th2.get(),
                                 fix.get(), out.get(), bad.get(), ni.get());
    };
    EXPECT(chk(off.get()) == nullptr);
    SAYS(chk(nullptr), "NULL pair_off");
    if (K >= 3) {
      off[2] = off[1] - 1;
      SAYS(chk(off.get()), "pair_off must not descend");
      off[2] = off[1] + kOptSim3HostMaxPairs + 1;
      SAYS(chk(off.get()), "more than 16384 pairs in one problem");
      off[2] = 14;
      th2[K - 1] = 0.0f;
      SAYS(chk(off.get()), "th2 must be positive and finite");
      th2[K - 1] = 10.0f;
    }
    off[0] = 1;
    SAYS(chk(off.get()), "pair_off[0] must be 0");
  }
  {
    int32_t off[1] = {0};
    SAYS(optsim3_check_multi(-1, off, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr), "negative problem count");
    SAYS(optsim3_check_multi(kOptSim3HostMaxProblems + 1, off, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr,
                             nullptr, nullptr, nullptr, nullptr, nullptr, nullptr), "more than 1048576 problems");
  }
  // the packing: every source and destination exactly as long as n says, every output element against its source.  16 pair
  // records fill a 256-byte line: counts that end just before, on and after one
  for (int n : {0, 1, 15, 16, 17, 31, 32, 33, 255, 256, 257, kOptSim3HostMaxPairs}) {
    auto x1 = exact<float>(3 * (size_t)n), x2 = exact<float>(3 * (size_t)n), o1 = exact<float>(2 * (size_t)n), o2 = exact<float>(2 * (size_t)n);
    auto w1 = exact<float>(n), w2 = exact<float>(n);
    for (int i = 0; i < n; i++) {
      for (int k = 0; k < 3; k++) { x1[3 * i + k] = (float)(3 * i + k) + 0.25f; x2[3 * i + k] = -(float)(3 * i + k) - 0.5f; }
      for (int k = 0; k < 2; k++) { o1[2 * i + k] = (float)(2 * i + k) + 0.125f; o2[2 * i + k] = (float)(2 * i + k) + 0.375f; }
      w1[i] = 1.0f / (float)(i + 1); w2[i] = 2.0f / (float)(i + 1);
    }
    auto A = exact<float>(4 * (size_t)n), B = exact<float>(4 * (size_t)n), C = exact<float>(4 * (size_t)n);
    for (size_t k = 0; k < 4 * (size_t)n; k++) A[k] = B[k] = C[k] = -7.0f;  // (no packed value is -7)
    optsim3_pack_pairs_a(A.get(), n, x1.get(), w1.get());
    optsim3_pack_pairs_b(B.get(), n, x2.get(), w2.get());
    optsim3_pack_pairs_c(C.get(), n, o1.get(), o2.get());
    for (int i = 0; i < n; i++) {
      EXPECT(A[4 * i] == x1[3 * i] && A[4 * i + 1] == x1[3 * i + 1] && A[4 * i + 2] == x1[3 * i + 2] && A[4 * i + 3] == w1[i]);
      EXPECT(B[4 * i] == x2[3 * i] && B[4 * i + 1] == x2[3 * i + 1] && B[4 * i + 2] == x2[3 * i + 2] && B[4 * i + 3] == w2[i]);
      EXPECT(C[4 * i] == o1[2 * i] && C[4 * i + 1] == o1[2 * i + 1] && C[4 * i + 2] == o2[2 * i] && C[4 * i + 3] == o2[2 * i + 1]);
      OptSim3Pair p;
      optsim3_unpack(A.get() + 4 * i, B.get() + 4 * i, C.get() + 4 * i, &p);
      EXPECT(p.X1[2] == (double)x1[3 * i + 2] && p.X2[0] == (double)x2[3 * i] && p.o2[1] == (double)o2[2 * i + 1] && p.w2 == (double)w2[i]);
    }
  }
  for (int K : {1, 5}) {
    auto off = exact<int32_t>((size_t)K + 1);
    auto c1 = exact<float>(4 * (size_t)K), c2 = exact<float>(4 * (size_t)K), s = exact<float>(13 * (size_t)K), th2 = exact<float>(K);
    auto fix = exact<uint8_t>(K);
    for (int p = 0; p < K; p++) {
      off[p + 1] = off[p] + 16 * p + 15;
      for (int k = 0; k < 4; k++) { c1[4 * p + k] = (float)(100 * p + k); c2[4 * p + k] = (float)(100 * p + k) + 0.5f; }
      for (int k = 0; k < 13; k++) s[13 * p + k] = (float)(p + k) * 0.25f;
      th2[p] = 10.0f + (float)p;
      fix[p] = (uint8_t)(p % 2 ? 7 : 0);
    }
    auto P = exact<OptSim3Problem>(K);
    optsim3_pack_problems(P.get(), K, off.get(), c1.get(), c2.get(), s.get(), th2.get(), fix.get());
    for (int p = 0; p < K; p++) {
      EXPECT(P[p].off == off[p] && P[p].n == 16 * p + 15 && P[p].cam1[3] == c1[4 * p + 3] && P[p].cam2[0] == c2[4 * p]);
      EXPECT(P[p].sim3[12] == s[13 * p + 12] && P[p].th2 == th2[p] && P[p].delta == std::sqrt(th2[p]) && P[p].fixScale == p % 2);
    }
  }
  std::printf("ok\n");
  return 0;
}
