// ransac_host_pins.cpp -- the host layers of the three RANSAC solvers (sim3_host.h, pnp_host.h, initializer_host.h) under
// their per-solver names, text for text: reads cases (tests/golden/ransac_host_pins.txt, written by
// tools/gen_ransac_host_pins.py) and writes one `out ...` line per case, in order.
//   ransac_host_pins <cases> <out>
// A case is one line `case <fn> <name> <int> ...`; every other line is skipped.  All values are decimal integers; a float
// travels as the 32-bit pattern of its value.
//   sim3_check / pnp_check / init_check, sim3_layout / pnp_layout / init_layout:
//       K N H nullmask  np pair_off[np]  nh hyp_off[nh]  <sets>  nf f[nf]
//     <sets> is `ns sets[ns]`, or `-1  r (n count start)[r]  p (index value)[p]`: r runs of `count` consecutive sets, set h
//     of a run being (start + h + i) % n for i < S, and then p single indices replaced.
//     f are the per-owner values: cam1[4K] cam2[4K] (sim3), cam[4K] (pnp), T1[4K] T2[4K] sigma[K] (init; T widened to
//     double).  Bit b of nullmask makes the b-th pointer argument of the check NULL, in the order of its signature.  Arrays
//     the checks only test for NULL are one dummy buffer.  pnp_check is pnp_check_common and, when that passes and H > 0,
//     pnp_check_sets, as orbfe_pnp_ransac* chains them.
//     *_check  -> the returned text, or `fine`
//     *_layout -> word_off, then every record's fields, then the owner of every item
//   draws3 / draws4 / draws8 (sim3_triples_from_draws, pnp_sets_from_draws, init_sets_from_draws):
//       n H nullmask  nd draws[nd]      (bit 0: draws NULL, bit 1: sets NULL)
//     -> `refused`, or `sets` and the H * S indices
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <string>
#include <vector>

#include "initializer_host.h"
#include "pnp_host.h"
#include "sim3_host.h"

using namespace orbfe;

static unsigned fbits(float f) { uint32_t b; memcpy(&b, &f, 4); return b; }
static unsigned long long dbits(double d) { uint64_t b; memcpy(&b, &d, 8); return b; }

struct Case {
  std::vector<long long> v;
  size_t at = 0;
  bool bad = false;
  long long next() {
    if (at >= v.size()) { bad = true; return 0; }
    return v[at++];
  }
  std::vector<int32_t> ints() {
    const long long n = next();
    std::vector<int32_t> a;
    for (long long i = 0; i < n && !bad; i++) a.push_back((int32_t)next());
    return a;
  }
  // the sets of a call: ns values, or -1 and runs of consecutive sets with single indices patched afterwards
  std::vector<int32_t> sets(int S) {
    if (at < v.size() && v[at] >= 0) return ints();
    next();
    std::vector<int32_t> a;
    for (long long runs = next(); runs > 0 && !bad; runs--) {
      const long long n = next(), count = next(), start = next();
      if (n <= 0) { bad = true; break; }
      for (long long h = 0; h < count; h++)
        for (int i = 0; i < S; i++) a.push_back((int32_t)((start + h + i) % n));
    }
    for (long long patches = next(); patches > 0 && !bad; patches--) {
      const long long i = next(), x = next();
      if (i < 0 || (size_t)i >= a.size()) { bad = true; break; }
      a[(size_t)i] = (int32_t)x;
    }
    return a;
  }
};

template <typename T>
static T* arg(unsigned mask, int bit, T* p) { return mask >> bit & 1u ? nullptr : p; }

int main(int argc, char** argv) {
  if (argc != 3) { fprintf(stderr, "usage: ransac_host_pins <cases> <out>\n"); return 2; }
  FILE* fi = fopen(argv[1], "r");
  FILE* fo = fopen(argv[2], "w");
  if (!fi || !fo) { fprintf(stderr, "ransac_host_pins: cannot open a file\n"); return 2; }
  static double dummy[4];  // stands for every array the checks only test for NULL
  float* df = reinterpret_cast<float*>(dummy);
  int32_t* di = reinterpret_cast<int32_t*>(dummy);
  uint8_t* db = reinterpret_cast<uint8_t*>(dummy);
  uint32_t* dw = reinterpret_cast<uint32_t*>(dummy);
  std::string line;
  int ch;
  for (;;) {
    line.clear();
    while ((ch = fgetc(fi)) != EOF && ch != '\n') line.push_back((char)ch);
    if (ch == EOF && line.empty()) break;
    char fn[64], name[128];
    int used = 0;
    if (sscanf(line.c_str(), "case %63s %127s%n", fn, name, &used) != 2) continue;
    Case c;
    const char* p = line.c_str() + used;
    for (;;) {
      char* end;
      const long long x = strtoll(p, &end, 10);
      if (end == p) break;
      c.v.push_back(x);
      p = end;
    }
    const std::string f = fn;
    std::string out;
    char buf[64];
    auto put = [&](long long x) { snprintf(buf, sizeof buf, " %lld", x); out += buf; };
    auto putu = [&](unsigned long long x) { snprintf(buf, sizeof buf, " %llu", x); out += buf; };
    if (f == "draws3" || f == "draws4" || f == "draws8") {
      const int n = (int)c.next(), H = (int)c.next();
      const unsigned mask = (unsigned)c.next();
      std::vector<int32_t> draws = c.ints();
      const int S = f == "draws3" ? 3 : f == "draws4" ? 4 : 8;
      if (c.bad || (H > 0 && draws.size() != (size_t)H * S)) { fprintf(stderr, "ransac_host_pins: %s %s: bad case\n", fn, name); return 2; }
      std::vector<int32_t> sets((size_t)(H > 0 ? H : 0) * S + 1, -7);
      int32_t* pd = arg(mask, 0, draws.empty() ? di : draws.data());
      int32_t* ps = arg(mask, 1, sets.data());
      const bool ok = S == 3 ? sim3_triples_from_draws(n, H, pd, ps) : S == 4 ? pnp_sets_from_draws(n, H, pd, ps) : init_sets_from_draws(n, H, pd, ps);
      out = ok ? " sets" : " refused";
      for (int i = 0; ok && i < H * S; i++) put(sets[i]);
    } else {
      const int K = (int)c.next(), N = (int)c.next(), H = (int)c.next();
      const unsigned mask = (unsigned)c.next();
      const int S = f.compare(0, 5, "sim3_") == 0 ? 3 : f.compare(0, 4, "pnp_") == 0 ? 4 : 8;
      std::vector<int32_t> poff = c.ints(), hoff = c.ints(), sets = c.sets(S), fb = c.ints();
      if (c.bad) { fprintf(stderr, "ransac_host_pins: %s %s: bad case\n", fn, name); return 2; }
      std::vector<float> fv(fb.size() + 1);
      for (size_t i = 0; i < fb.size(); i++) { const uint32_t b = (uint32_t)fb[i]; memcpy(&fv[i], &b, 4); }
      std::vector<int32_t> word_off((size_t)(K > 0 ? K : 0) + 1, -7), owner;
      if (sets.empty()) sets.push_back(0);
      const bool layout = f.size() > 7 && f.compare(f.size() - 7, 7, "_layout") == 0;
      const size_t k4 = 4 * (size_t)(K > 0 ? K : 0);
      if (f.compare(0, 5, "sim3_") == 0) {
        if (fb.size() != 2 * k4 && !fb.empty()) { fprintf(stderr, "ransac_host_pins: %s: bad f\n", name); return 2; }
        const float *cam1 = fv.data(), *cam2 = fv.data() + (fb.empty() ? 0 : k4);
        if (!layout) {
          const char* e = sim3_check(K, N, H, arg(mask, 0, poff.data()), arg(mask, 1, df), arg(mask, 2, df), arg(mask, 3, df),
                                     arg(mask, 4, df), arg(mask, 5, cam1), arg(mask, 6, cam2), arg(mask, 7, hoff.data()),
                                     arg(mask, 8, sets.data()), arg(mask, 9, di), arg(mask, 10, db), arg(mask, 11, df),
                                     arg(mask, 12, dw), arg(mask, 13, word_off.data()));
          out = std::string(" ") + (e ? e : "fine");
        } else {
          std::vector<Sim3Candidate> r;
          sim3_layout(K, poff.data(), hoff.data(), cam1, cam2, word_off.data(), &r, &owner);
          out = " word_off";
          for (int32_t w : word_off) put(w);
          for (const Sim3Candidate& q : r) {
            out += " rec";
            put(q.pair0); put(q.nPairs); put(q.hyp0); put(q.word0); put(q.words);
            putu(fbits(q.K1.fx)); putu(fbits(q.K1.fy)); putu(fbits(q.K1.cx)); putu(fbits(q.K1.cy));
            putu(fbits(q.K2.fx)); putu(fbits(q.K2.fy)); putu(fbits(q.K2.cx)); putu(fbits(q.K2.cy));
          }
        }
      } else if (f.compare(0, 4, "pnp_") == 0) {
        if (fb.size() != k4 && !fb.empty()) { fprintf(stderr, "ransac_host_pins: %s: bad f\n", name); return 2; }
        const float* cam = fv.data();
        if (!layout) {
          const char* e = pnp_check_common(K, N, H, arg(mask, 0, poff.data()), arg(mask, 1, df), arg(mask, 2, df), arg(mask, 3, df),
                                           arg(mask, 4, cam), arg(mask, 5, hoff.data()), arg(mask, 6, (const void*)sets.data()),
                                           arg(mask, 7, di), arg(mask, 8, db), arg(mask, 9, df), arg(mask, 10, word_off.data()),
                                           arg(mask, 11, dw));
          if (!e && H > 0) e = pnp_check_sets(K, poff.data(), hoff.data(), sets.data());
          out = std::string(" ") + (e ? e : "fine");
        } else {
          std::vector<PnpCandidate> r;
          pnp_layout(K, poff.data(), hoff.data(), cam, word_off.data(), &r, &owner);
          out = " word_off";
          for (int32_t w : word_off) put(w);
          for (const PnpCandidate& q : r) {
            out += " rec";
            put(q.point0); put(q.nPoints); put(q.hyp0); put(q.word0); put(q.words);
            putu(fbits(q.K.fu)); putu(fbits(q.K.fv)); putu(fbits(q.K.uc)); putu(fbits(q.K.vc));
          }
        }
      } else if (f.compare(0, 5, "init_") == 0) {
        if (fb.size() != 2 * k4 + k4 / 4 && !fb.empty()) { fprintf(stderr, "ransac_host_pins: %s: bad f\n", name); return 2; }
        std::vector<double> T(2 * k4 + 1);
        for (size_t i = 0; i < 2 * k4 && !fb.empty(); i++) T[i] = (double)fv[i];
        const double *T1 = T.data(), *T2 = T.data() + k4;
        const float* sigma = fv.data() + (fb.empty() ? 0 : 2 * k4);
        if (!layout) {
          const char* e = init_check(K, N, H, arg(mask, 0, poff.data()), arg(mask, 1, df), arg(mask, 2, T1), arg(mask, 3, T2),
                                     arg(mask, 4, sigma), arg(mask, 5, hoff.data()), arg(mask, 6, sets.data()), arg(mask, 7, dummy),
                                     arg(mask, 8, db), arg(mask, 9, di), arg(mask, 10, dummy), arg(mask, 11, dummy), arg(mask, 12, dw),
                                     arg(mask, 13, word_off.data()));
          out = std::string(" ") + (e ? e : "fine");
        } else {
          std::vector<InitProblem> r;
          init_layout(K, poff.data(), hoff.data(), T1, T2, sigma, word_off.data(), &r, &owner);
          out = " word_off";
          for (int32_t w : word_off) put(w);
          for (const InitProblem& q : r) {
            out += " rec";
            put(q.pair0); put(q.nPairs); put(q.hyp0); put(q.word0); put(q.words);
            putu(fbits(q.sigma));
            for (int i = 0; i < 4; i++) putu(dbits(q.T1[i]));
            for (int i = 0; i < 4; i++) putu(dbits(q.T2[i]));
          }
        }
      } else {
        fprintf(stderr, "ransac_host_pins: unknown function %s\n", fn);
        return 2;
      }
      if (layout) {
        out += " owner";
        for (int32_t k : owner) put(k);
      }
    }
    fprintf(fo, "out%s\n", out.c_str());
  }
  fclose(fo);
  fclose(fi);
  return 0;
}
