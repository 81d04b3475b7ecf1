// Stand-alone program for the address and undefined-behaviour sanitizers (tests/test_sim3_host_san.py): the host side of
// orbfe_sim3_ransac* that needs no device -- csrc/sim3_host.h (checks, layout, triples_from_draws, max_iterations),
// csrc/sim3_math.h and the replay of include/orbfe_sim3_replay.hpp -- with every array exactly as long as the call says, so
// that a read or write past an end is an error.  Prints "ok".
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <memory>
#include <string>
#include <vector>

#include "../../include/orbfe_sim3_replay.hpp"
#include "sim3_host.h"

using namespace orbfe;

namespace {
int failures = 0;
void expect(bool ok, const char* what) {
  if (!ok) { std::printf("FAILED: %s\n", what); failures++; }
}
// an array of exactly n elements on the heap (n = 0: a one-byte block nobody may touch)
template <typename T>
std::unique_ptr<T[]> exact(const std::vector<T>& v) {
  std::unique_ptr<T[]> p(new T[v.size() ? v.size() : 1]);
  for (size_t i = 0; i < v.size(); i++) p[i] = v[i];
  return p;
}

struct Call {
  int K, N, H;
  std::vector<int32_t> pairOff, hypOff, triples;
  std::vector<float> x1, x2, e1, e2, c1, c2;
  const char* check(bool nullTriples = false) const {
    auto po = exact(pairOff), ho = exact(hypOff), tr = exact(triples);
    auto a = exact(x1), b = exact(x2), c = exact(e1), d = exact(e2), k1 = exact(c1), k2 = exact(c2);
    std::unique_ptr<int32_t[]> ni(new int32_t[H ? H : 1]), wo(new int32_t[K + 1]);
    std::unique_ptr<uint8_t[]> st(new uint8_t[H ? H : 1]);
    std::unique_ptr<float[]> s3(new float[H ? 13 * H : 1]);
    std::unique_ptr<uint32_t[]> w(new uint32_t[1]);
    return sim3_check(K, N, H, po.get(), a.get(), b.get(), c.get(), d.get(), k1.get(), k2.get(), ho.get(),
                      nullTriples ? nullptr : tr.get(), ni.get(), st.get(), s3.get(), w.get(), wo.get());
  }
};

Call good() {
  Call c;
  c.K = 3; c.N = 3 + 40 + 33; c.H = 2 + 0 + 3;
  c.pairOff = {0, 3, 43, 76}; c.hypOff = {0, 2, 2, 5};
  c.triples = {0, 1, 2, 2, 0, 1, 0, 32, 5, 31, 30, 29, 1, 2, 3};
  for (int i = 0; i < c.N; i++) {
    const float x = 0.1f * (float)(i % 7) - 0.3f, y = 0.07f * (float)(i % 5) - 0.1f, z = 2.0f + 0.05f * (float)(i % 11);
    c.x2.insert(c.x2.end(), {x, y, z});
    c.x1.insert(c.x1.end(), {1.3f * x + 0.3f, 1.3f * y - 0.2f, 1.3f * z + 0.4f});
    c.e1.push_back(9.21f); c.e2.push_back(13.26f);
  }
  for (int k = 0; k < 3; k++) { c.c1.insert(c.c1.end(), {517.3f, 516.5f, 318.6f, 255.3f}); c.c2.insert(c.c2.end(), {520.9f, 521.0f, 325.1f, 249.7f}); }
  return c;
}
}  // namespace

// `triples n H`: H * 3 draws on standard input -> the triples; `maxits`: n min_inliers max_its per line -> the iterations.
// For tests/test_sim3_host_san.py to compare with tests/sim3_ref.py on more inputs than the lists below.
int filter(int argc, char** argv) {
  if (std::string(argv[1]) == "triples" && argc == 4) {
    const int n = std::atoi(argv[2]), H = std::atoi(argv[3]);
    std::unique_ptr<int32_t[]> d(new int32_t[H > 0 ? 3 * H : 1]), t(new int32_t[H > 0 ? 3 * H : 1]);
    for (int i = 0; i < 3 * H; i++)
      if (std::scanf("%d", &d[i]) != 1) return 2;
    if (!sim3_triples_from_draws(n, H, d.get(), t.get())) { std::printf("refused\n"); return 0; }
    for (int i = 0; i < 3 * H; i++) std::printf("%d ", t[i]);
    std::printf("\n");
    return 0;
  }
  if (std::string(argv[1]) == "maxits") {
    int n, mi, mx;
    while (std::scanf("%d %d %d", &n, &mi, &mx) == 3) std::printf("%d\n", sim3_max_iterations(n, 0.99, mi, mx));
    return 0;
  }
  return 2;
}

int main(int argc, char** argv) {
  if (argc > 1) return filter(argc, argv);
  // ---- checks ----
  expect(good().check() == nullptr, "a good call passes");
  { Call c = good(); c.pairOff[1] = 44; expect(c.check() != nullptr, "pair_off not monotone"); }
  { Call c = good(); c.N--; expect(c.check() != nullptr, "pair_off does not end at N"); }
  { Call c = good(); c.H++; expect(c.check() != nullptr, "hyp_off does not end at H"); }
  { Call c = good(); c.hypOff[0] = 1; expect(c.check() != nullptr, "hyp_off does not start at 0"); }
  { Call c = good(); c.triples[2] = 3; expect(c.check() != nullptr, "triple index == n_k"); }
  { Call c = good(); c.triples[7] = -1; expect(c.check() != nullptr, "negative triple index"); }
  { Call c = good(); c.triples[14] = c.triples[12]; expect(c.check() != nullptr, "repeated index"); }
  { Call c = good(); c.c1[5] = std::numeric_limits<float>::quiet_NaN(); expect(c.check() != nullptr, "NaN camera"); }
  { Call c = good(); c.c2[11] = std::numeric_limits<float>::infinity(); expect(c.check() != nullptr, "infinite camera"); }
  { Call c = good(); c.pairOff = {0, 2, 43, 76}; c.triples[2] = 1; expect(std::string(c.check()) == "a candidate with fewer than 3 pairs has hypotheses", "n_k < 3 with hypotheses"); }
  { Call c = good(); expect(c.check(true) != nullptr, "NULL triples"); }
  { Call c = good(); c.K = -1; expect(c.check() != nullptr, "negative K"); }
  { Call c; c.K = 0; c.N = 0; c.H = 0; c.pairOff = {0}; c.hypOff = {0}; expect(c.check() == nullptr, "an empty call is legal"); }
  // ---- layout ----
  {
    const Call c = good();
    auto po = exact(c.pairOff), ho = exact(c.hypOff);
    auto k1 = exact(c.c1), k2 = exact(c.c2);
    std::unique_ptr<int32_t[]> wo(new int32_t[c.K + 1]);
    std::vector<Sim3Candidate> cands;
    std::vector<int32_t> hypCand;
    sim3_layout(c.K, po.get(), ho.get(), k1.get(), k2.get(), wo.get(), &cands, &hypCand);
    expect(wo[0] == 0 && wo[1] == 2 && wo[2] == 2 && wo[3] == 2 + 3 * 2, "word offsets");
    expect(hypCand == std::vector<int32_t>({0, 0, 2, 2, 2}), "candidate of every hypothesis");
    expect(cands.size() == 3 && cands[2].pair0 == 43 && cands[2].nPairs == 33 && cands[2].words == 2 && cands[2].hyp0 == 2 && cands[2].word0 == 2, "candidate record");
    // ---- the arithmetic on exactly-sized arrays: an exact triple of candidate 2 finds every pair of it ----
    auto x1 = exact(c.x1), x2 = exact(c.x2);
    float P1[3][3], P2[3][3];
    const int tri[3] = {0, 32, 5};
    for (int j = 0; j < 3; j++)
      for (int i = 0; i < 3; i++) { P1[j][i] = x1[3 * (43 + tri[j]) + i]; P2[j][i] = x2[3 * (43 + tri[j]) + i]; }
    Sim3Transform T;
    sim3_compute(P1, P2, false, &T);
    expect(!sim3_nonfinite(T) && std::fabs(T.s - 1.3) < 1e-5 && std::fabs(T.R[0] - 1.0) < 1e-5 && std::fabs(T.t[2] - 0.4) < 1e-4, "planted scale and translation");
    int inl = 0;
    for (int i = 0; i < 33; i++) inl += sim3_is_inlier(T, cands[2].K1, cands[2].K2, &x1[3 * (43 + i)], &x2[3 * (43 + i)], 9.21f, 13.26f);
    expect(inl == 33, "every pair is an inlier of the planted transform");
    sim3_compute(P2, P2, false, &T);  // identical sets: the reference's division by |vec| = 0
    expect(sim3_nonfinite(T) && std::isnan(T.R[0]), "identical sets are NONFINITE");
    expect(!sim3_is_inlier(T, cands[2].K1, cands[2].K2, &x1[0], &x2[0], 9.21f, 13.26f), "NaN compares false");
  }
  // ---- triples_from_draws ----
  {
    const std::vector<int32_t> draws = {0, 0, 0, 6, 5, 4, 6, 0, 0, 3, 3, 3, 0, 5, 0};
    auto d = exact(draws);
    std::unique_ptr<int32_t[]> t(new int32_t[15]);
    expect(sim3_triples_from_draws(7, 5, d.get(), t.get()), "draws accepted");
    const int32_t want[15] = {0, 6, 5, 6, 5, 4, 6, 0, 5, 3, 6, 5, 0, 5, 6};
    bool same = true;
    for (int i = 0; i < 15; i++) same = same && t[i] == want[i];
    expect(same, "triples as the list-pop gives them");
    const std::vector<int32_t> bad = {0, 6, 0};
    auto b = exact(bad);
    expect(!sim3_triples_from_draws(7, 1, b.get(), t.get()), "second draw indexes a list of 6");
    expect(!sim3_triples_from_draws(2, 1, d.get(), t.get()), "fewer than 3 pairs");
    expect(sim3_triples_from_draws(2, 0, nullptr, nullptr), "no hypotheses need no arrays");
  }
  // ---- max_iterations ----
  expect(sim3_max_iterations(100, 0.99, 20, 300) == 300 && sim3_max_iterations(40, 0.99, 20, 300) == 35 &&
             sim3_max_iterations(25, 0.99, 20, 300) == 7 && sim3_max_iterations(21, 0.99, 20, 300) == 3 &&
             sim3_max_iterations(40, 0.99, 20, 10) == 10, "hand-computed iteration counts");
  expect(sim3_max_iterations(20, 0.99, 20, 300) == 1 && sim3_max_iterations(19, 0.99, 20, 300) == 1 &&
             sim3_max_iterations(0, 0.99, 6, 300) == 1 && sim3_max_iterations(1000000, 0.99, 1, 300) == 1 &&
             sim3_max_iterations(10, 0.99, 0, 300) == 1, "N == minInliers, N < minInliers and the edges of the formula");
  // ---- the replay ----
  {
    using orbfe_cpp::Sim3Replay;
    const int N = 33;  // two words, the second with one pair
    const std::vector<int32_t> counts = {3, 20, 20, 21, 33, 0};
    std::vector<uint32_t> words;
    for (int32_t c : counts) { words.push_back(c >= 32 ? 0xFFFFFFFFu : (1u << c) - 1u); words.push_back(c > 32 ? 1u : 0u); }
    std::vector<int32_t> idx;
    for (int i = 0; i < N; i++) idx.push_back(2 * i + 1);
    auto n = exact(counts); auto w = exact(words); auto ix = exact(idx);
    Sim3Replay s;
    s.N = N; s.mN1 = 2 * N; s.mRansacMinInliers = 20; s.mRansacMaxIts = 6;
    std::vector<bool> vb;
    Sim3Replay::Step r = s.iterate(5, n.get(), w.get(), ix.get(), vb);
    int set = 0;
    for (size_t i = 0; i < vb.size(); i++) set += vb[i] && (i % 2 == 1) && i < 42;
    expect(r.accepted == 3 && r.best == 3 && !r.bNoMore && r.nInliers == 21 && set == 21 && s.mnIterations == 4 && vb.size() == 66, "first count above min, == min passed over");
    r = s.iterate(5, n.get(), w.get(), ix.get(), vb);
    expect(r.accepted == 4 && r.best == 4 && r.nInliers == 33 && vb[65] && s.mnBestInliers == 33, "a later acceptance; the pair of the second word");
    r = s.iterate(5, n.get(), w.get(), ix.get(), vb);
    expect(r.accepted < 0 && r.best < 0 && r.bNoMore && s.mnIterations == 6, "bNoMore on the last iteration; no new best, no index");
    // re-parameterised to FEWER hypotheses (SetRansacParameters: mnIterations = 0, mnBestInliers kept, :141) and evaluated
    // anew: the arrays hold 2 hypotheses now, and nothing of the old list -- whose best was index 4 -- may be read
    const std::vector<int32_t> counts2 = {32, 33};
    const std::vector<uint32_t> words2 = {0xFFFFFFFFu, 0u, 0xFFFFFFFFu, 1u};
    auto n2 = exact(counts2); auto w2 = exact(words2);
    s.mRansacMaxIts = 2; s.mnIterations = 0;
    r = s.iterate(1, n2.get(), w2.get(), ix.get(), vb);
    expect(r.accepted < 0 && r.best < 0 && !r.bNoMore && s.mnBestInliers == 33, "below the best kept across the re-evaluation: not taken");
    r = s.iterate(5, n2.get(), w2.get(), ix.get(), vb);
    expect(r.accepted == 1 && r.best == 1 && s.mnIterations == 2, "the new list's own index is reported");
    s.mRansacMinInliers = 40; s.mnIterations = 0;  // minInliers above N: no hypotheses at all
    r = s.iterate(5, nullptr, nullptr, ix.get(), vb);
    expect(r.bNoMore && r.best < 0 && r.accepted < 0, "minInliers above N after a use");
    Sim3Replay few;
    few.N = 5; few.mN1 = 9; few.mRansacMinInliers = 6; few.mRansacMaxIts = 1;
    r = few.iterate(5, nullptr, nullptr, nullptr, vb);
    expect(r.bNoMore && r.accepted < 0 && few.mnIterations == 0 && vb.size() == 9, "N < minInliers touches nothing");
    expect(orbfe_cpp::sim3_seeded_draw(7, 0, 10) >= 0 && orbfe_cpp::sim3_seeded_draw(7, 0, 10) < 10 &&
               orbfe_cpp::sim3_seeded_draw(0xFFFFFFFFFFFFFFFFull, 5, 1) == 0, "seeded draws stay in range");
  }
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
