// Stand-alone program for the address and undefined-behaviour sanitizers: the host side of orbfe_pnp_* that needs no device
// -- csrc/pnp_host.h (every refusal, the layout, the compaction of record masks, the record scan, sets_from_draws), the
// arithmetic of csrc/pnp_math.h on one scene, and PnPReplay of include/orbfe_pnp_replay.hpp on hand-made count sequences --
// with every array on the heap and exactly as long as the call says.  Prints "ok".  With arguments: "draws n H" reads 4 H
// draws from stdin and prints the sets; "params" reads lines "N prob minInliers maxIts epsilon" and prints minInliers maxIts.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include "../../include/orbfe_pnp_replay.hpp"
#include "pnp_host.h"

using namespace orbfe;

#define EXPECT(cond)                                                        \
  do {                                                                      \
    if (!(cond)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

namespace {

struct Call {  // a valid ransac call on K = 2 candidates of 40 and 33 correspondences with 3 and 2 hypotheses
  std::vector<int32_t> pointOff{0, 40, 73}, hypOff{0, 3, 5}, sets{0, 1, 2, 3, 39, 5, 6, 7, 10, 20, 30, 38, 0, 1, 2, 32, 4, 5, 6, 7};
  std::vector<float> p3d = std::vector<float>(73 * 3, 1.f), p2d = std::vector<float>(73 * 2, 2.f), maxErr = std::vector<float>(73, 6.f);
  std::vector<float> cam{500.f, 500.f, 320.f, 240.f, 400.f, 400.f, 300.f, 200.f};
  std::vector<int32_t> nInl = std::vector<int32_t>(5), wordOff = std::vector<int32_t>(3);
  std::vector<uint8_t> status = std::vector<uint8_t>(5);
  std::vector<float> pose = std::vector<float>(60);
  std::vector<uint32_t> words = std::vector<uint32_t>(3 * 2 + 2 * 2);
  const char* check(int K = 2, int N = 73, int H = 5) {
    const char* e = pnp_check_common(K, N, H, pointOff.data(), p3d.data(), p2d.data(), maxErr.data(), cam.data(), hypOff.data(),
                                     sets.data(), nInl.data(), status.data(), pose.data(), wordOff.data(), words.data());
    if (!e && H > 0) e = pnp_check_sets(K, pointOff.data(), hypOff.data(), sets.data());
    return e;
  }
};

int refusals() {
  { Call c; EXPECT(!c.check()); }
  { Call c; EXPECT(c.check(-1)); EXPECT(c.check(4097)); }  // n_candidates outside [0, 4096], before any array is read
  { Call c; EXPECT(c.check(2, -1)); EXPECT(c.check(2, 73, -1)); }
  // NULL arrays, one at a time
  {
    Call c;
    const float* fnull = nullptr;
    const int32_t* inull = nullptr;
    EXPECT(pnp_check_common(2, 73, 5, inull, c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), fnull, c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), fnull, c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), fnull, c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), fnull, c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), inull, c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), nullptr, c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), inull, c.status.data(), c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), nullptr, c.pose.data(), c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), fnull, c.wordOff.data(), c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), inull, c.words.data()));
    EXPECT(pnp_check_common(2, 73, 5, c.pointOff.data(), c.p3d.data(), c.p2d.data(), c.maxErr.data(), c.cam.data(), c.hypOff.data(), c.sets.data(), c.nInl.data(), c.status.data(), c.pose.data(), c.wordOff.data(), nullptr));
  }
  // offsets: not from 0, decreasing, not ending at the totals
  { Call c; c.pointOff[0] = 1; EXPECT(c.check()); }
  { Call c; c.pointOff = {0, 80, 73}; EXPECT(c.check()); }
  { Call c; c.pointOff[2] = 72; EXPECT(c.check()); }
  { Call c; c.hypOff[0] = 1; EXPECT(c.check()); }
  { Call c; c.hypOff = {0, 6, 5}; EXPECT(c.check()); }
  { Call c; c.hypOff[2] = 4; EXPECT(c.check()); }
  // sets: outside [0, n_k) (40 is outside candidate 0, 33 outside candidate 1), negative, repeated
  { Call c; c.sets[4] = 40; EXPECT(c.check()); }
  { Call c; c.sets[15] = 33; EXPECT(c.check()); }
  { Call c; c.sets[0] = -1; EXPECT(c.check()); }
  { Call c; c.sets[3] = c.sets[0]; EXPECT(c.check()); }
  // camera
  { Call c; c.cam[5] = INFINITY; EXPECT(c.check()); }
  { Call c; c.cam[0] = NAN; EXPECT(c.check()); }
  // a candidate with n_k < 4 that has hypotheses; without hypotheses it is legal
  { Call c; c.pointOff = {0, 3, 73}; c.sets.assign(20, 0); EXPECT(c.check()); }
  { Call c; c.pointOff = {0, 3, 73}; c.hypOff = {0, 0, 5}; for (int h = 0; h < 5; h++) for (int i = 0; i < 4; i++) c.sets[4 * h + i] = i + h; EXPECT(!c.check()); }
  // nothing to do
  { Call c; c.hypOff = {0, 0, 0}; EXPECT(!c.check(2, 73, 0)); }
  {
    const int32_t off0[1] = {0};
    int32_t wo[1];
    EXPECT(!pnp_check_common(0, 0, 0, off0, nullptr, nullptr, nullptr, nullptr, off0, nullptr, nullptr, nullptr, nullptr, wo, nullptr));
  }
  // record masks: fewer than 4 bits, a bit at n_k, bits beyond n_k in the last word
  {
    const std::vector<int32_t> pointOff{0, 40}, recOff{0, 2};
    std::vector<uint32_t> m{0xFu, 0u, 0x80000001u, 0x82u};
    EXPECT(!pnp_check_masks(1, pointOff.data(), recOff.data(), m.data()));
    m[0] = 0x7u;
    EXPECT(pnp_check_masks(1, pointOff.data(), recOff.data(), m.data()));
    m[0] = 0xFu; m[3] = 0x182u;  // bit 8 of word 1 = correspondence 40
    EXPECT(pnp_check_masks(1, pointOff.data(), recOff.data(), m.data()));
    m[3] = 0x80000082u;
    EXPECT(pnp_check_masks(1, pointOff.data(), recOff.data(), m.data()));
    const std::vector<int32_t> p64{0, 64};  // n_k a multiple of 32: every bit of the last word is a correspondence
    std::vector<uint32_t> full{0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0xF0000000u};
    EXPECT(!pnp_check_masks(1, p64.data(), recOff.data(), full.data()));
  }
  // orbfe_pnp_solve_multi's own arguments
  {
    const std::vector<int32_t> mi{10, 4};
    std::vector<int32_t> ro(3), rh(5), rn(5), rwo(3);
    std::vector<uint8_t> rs(5);
    std::vector<float> rp(60);
    std::vector<uint32_t> rw(10);
    EXPECT(!pnp_check_solve(2, 5, mi.data(), ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, nullptr, ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(4097, 5, nullptr, ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(-1, 5, mi.data(), ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), nullptr, rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), ro.data(), nullptr, rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), ro.data(), rh.data(), nullptr, rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), ro.data(), rh.data(), rn.data(), nullptr, rp.data(), rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), ro.data(), rh.data(), rn.data(), rs.data(), nullptr, rwo.data(), rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), nullptr, rw.data()));
    EXPECT(pnp_check_solve(2, 5, mi.data(), ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), nullptr));
    const std::vector<int32_t> low{10, 3};
    EXPECT(pnp_check_solve(2, 5, low.data(), ro.data(), rh.data(), rn.data(), rs.data(), rp.data(), rwo.data(), rw.data()));
    EXPECT(!pnp_check_solve(2, 0, mi.data(), ro.data(), nullptr, nullptr, nullptr, nullptr, rwo.data(), nullptr));
  }
  return 0;
}

int layout_scan_compact() {
  Call c;
  std::vector<PnpCandidate> cands;
  std::vector<int32_t> hypCand;
  pnp_layout(2, c.pointOff.data(), c.hypOff.data(), c.cam.data(), c.wordOff.data(), &cands, &hypCand);
  EXPECT(c.wordOff[0] == 0 && c.wordOff[1] == 6 && c.wordOff[2] == 10);
  EXPECT(cands.size() == 2 && cands[1].point0 == 40 && cands[1].nPoints == 33 && cands[1].hyp0 == 3 && cands[1].word0 == 6 && cands[1].words == 2);
  EXPECT(cands[1].K.fu == 400.f && cands[1].K.vc == 200.f);
  EXPECT((hypCand == std::vector<int32_t>{0, 0, 0, 1, 1}));
  // the record scan: >= minInliers AND above every earlier qualifying count -- ties are no record, a count equal to
  // minInliers is one, counts below minInliers never are however large the prefix
  const std::vector<int32_t> hypOff{0, 9, 9, 13}, counts{3, 9, 10, 10, 12, 11, 12, 30, 30, /* */ 4, 4, 5, 3}, minInl{10, 10, 4};
  std::vector<int32_t> recOff(4), rec;
  pnp_scan_records(3, hypOff.data(), counts.data(), minInl.data(), recOff.data(), &rec);
  EXPECT((rec == std::vector<int32_t>{2, 4, 7, 9, 11}));
  EXPECT(recOff[0] == 0 && recOff[1] == 3 && recOff[2] == 3 && recOff[3] == 5);
  // compaction: the set bits ascending, record after record
  const std::vector<int32_t> pointOff{0, 40, 73}, recOff2{0, 1, 3};
  const std::vector<uint32_t> masks{0x80000003u, 0x81u, /* */ 0xFu, 0x0u, 0x10000000u, 0x1u};
  std::vector<int32_t> idxOff, idx;
  pnp_compact(2, pointOff.data(), recOff2.data(), masks.data(), &idxOff, &idx);
  EXPECT((idxOff == std::vector<int32_t>{0, 5, 9, 11}));
  EXPECT((idx == std::vector<int32_t>{0, 1, 31, 32, 39, 0, 1, 2, 3, 28, 32}));
  // sets_from_draws
  const std::vector<int32_t> draws{0, 0, 0, 0, 9, 8, 7, 6, 3, 3, 3, 3};
  std::vector<int32_t> sets(12);
  EXPECT(pnp_sets_from_draws(10, 3, draws.data(), sets.data()));
  EXPECT((sets == std::vector<int32_t>{0, 9, 8, 7, 9, 8, 7, 6, 3, 9, 8, 7}));
  const std::vector<int32_t> bad{0, 0, 0, 7};
  EXPECT(!pnp_sets_from_draws(10, 1, bad.data(), sets.data()));
  EXPECT(!pnp_sets_from_draws(3, 1, draws.data(), sets.data()));
  EXPECT(!pnp_sets_from_draws(10, 1, nullptr, sets.data()));
  EXPECT(pnp_sets_from_draws(10, 0, nullptr, nullptr));
  return 0;
}

// the arithmetic on a planted pose: every array indexed inside PnpWork or on the heap
struct HeapPoints {
  std::vector<float> p3d, p2d;
  std::vector<int32_t> idx;
  int n() const { return (int)idx.size(); }
  void get(int i, double pw[3], double uv[2]) const {
    const size_t p = (size_t)idx[(size_t)i];
    pw[0] = p3d[3 * p]; pw[1] = p3d[3 * p + 1]; pw[2] = p3d[3 * p + 2];
    uv[0] = p2d[2 * p]; uv[1] = p2d[2 * p + 1];
  }
};

int arithmetic() {
  const PnpCamera K = {500.f, 510.f, 320.f, 240.f};
  HeapPoints P;
  const double t[3] = {0.1, -0.2, 0.3};
  for (int i = 0; i < 37; i++) {
    const double x = ((i * 37) % 23) / 5.0 - 2.0, y = ((i * 53) % 19) / 5.0 - 1.8, z = 3.0 + ((i * 29) % 17) / 3.0;
    P.p3d.push_back((float)x); P.p3d.push_back((float)y); P.p3d.push_back((float)z);
    const double X = (double)(float)x + t[0], Y = (double)(float)y + t[1], Z = (double)(float)z + t[2];  // R = I
    P.p2d.push_back((float)(K.uc + K.fu * X / Z)); P.p2d.push_back((float)(K.vc + K.fv * Y / Z));
    P.idx.push_back(i);
  }
  std::vector<PnpWork> W(1);
  double R[9], tt[3];
  pnp_compute_pose(P, K, W.data(), R, tt);
  EXPECT(!pnp_nonfinite(R, tt));
  EXPECT(fabs(R[0] - 1.0) < 1e-4 && fabs(R[4] - 1.0) < 1e-4 && fabs(R[8] - 1.0) < 1e-4);
  EXPECT(fabs(tt[0] - t[0]) < 1e-3 && fabs(tt[1] - t[1]) < 1e-3 && fabs(tt[2] - t[2]) < 1e-3);
  int count = 0;
  for (int i = 0; i < 37; i++) count += pnp_is_inlier(R, tt, K, &P.p3d[3 * (size_t)i], &P.p2d[2 * (size_t)i], 5.991f);
  EXPECT(count == 37);
  P.idx = {0, 11, 22, 33};  // the minimal problem: whatever it finds, it reads and writes inside its arrays
  pnp_compute_pose(P, K, W.data(), R, tt);
  P.p3d[3 * 11] = P.p3d[0]; P.p3d[3 * 11 + 1] = P.p3d[1]; P.p3d[3 * 11 + 2] = P.p3d[2];  // two identical points
  pnp_compute_pose(P, K, W.data(), R, tt);
  for (int i = 0; i < 4; i++) P.p3d[3 * (size_t)P.idx[(size_t)i] + 2] = 4.f;  // coplanar
  pnp_compute_pose(P, K, W.data(), R, tt);
  for (int i = 0; i < 4; i++) for (int j = 0; j < 3; j++) P.p3d[3 * (size_t)P.idx[(size_t)i] + j] = 1.f;  // one point four times
  pnp_compute_pose(P, K, W.data(), R, tt);
  (void)pnp_nonfinite(R, tt);
  return 0;
}

struct Results {  // a solver of N = 40 correspondences: hypotheses with the given counts, records from the scan
  std::vector<int32_t> counts, recHyp, recCounts, kp;
  std::vector<uint32_t> words, recWords;
  Results(const std::vector<int32_t>& c, int minInliers, const std::vector<int32_t>& refined) : counts(c) {
    const std::vector<int32_t> hypOff{0, (int32_t)c.size()}, mi{minInliers};
    std::vector<int32_t> recOff(2);
    pnp_scan_records(1, hypOff.data(), counts.data(), mi.data(), recOff.data(), &recHyp);
    recCounts = refined;
    recCounts.resize(recHyp.size(), 0);
    for (int32_t n : counts) push(&words, n);
    for (int32_t n : recCounts) push(&recWords, n);
    for (int i = 0; i < 40; i++) kp.push_back(2 * i + 1);
  }
  static void push(std::vector<uint32_t>* w, int n) {  // the first n correspondences
    w->push_back(n >= 32 ? 0xFFFFFFFFu : ((1u << n) - 1u));
    w->push_back(n > 32 ? ((1u << (n - 32)) - 1u) : 0u);
  }
  orbfe_cpp::PnPReplay::Step iterate(orbfe_cpp::PnPReplay* st, int nIterations, std::vector<bool>* vb) {
    return st->iterate(nIterations, (int)counts.size(), counts.data(), words.data(), (int)recHyp.size(), recHyp.data(),
                       recCounts.data(), recWords.data(), kp.data(), *vb);
  }
};

int count_true(const std::vector<bool>& v) {
  int n = 0;
  for (bool b : v) n += b;
  return n;
}

int replay() {
  using orbfe_cpp::PnPReplay;
  // SetRansacParameters for (0.99, 10, 300, 4, 0.5) at N = 4, 10, 19, 20, 21, 100
  const int Ns[6] = {4, 10, 19, 20, 21, 100}, wantMin[6] = {10, 10, 10, 10, 10, 50}, wantIts[6] = {1, 1, 30, 35, 35, 35};
  for (int i = 0; i < 6; i++) {
    PnPReplay st;
    st.N = Ns[i];
    st.SetRansacParameters(0.99, 10, 300, 4, 0.5f);
    EXPECT(st.mRansacMinInliers == wantMin[i] && st.mRansacMaxIts == wantIts[i]);
  }
  std::vector<bool> vb;
  auto fresh = [](int minInliers, int maxIts) {
    PnPReplay st;
    st.N = 40; st.nKeyPoints = 83; st.mRansacMinInliers = minInliers; st.mRansacMaxIts = maxIts;
    return st;
  };
  {  // N < minInliers: bNoMore at once (:186), nothing is read
    PnPReplay st = fresh(41, 5);
    const PnPReplay::Step r = st.iterate(5, 0, nullptr, nullptr, 0, nullptr, nullptr, nullptr, nullptr, vb);
    EXPECT(r.bNoMore && r.refined < 0 && r.best < 0 && vb.empty() && st.mnIterations == 0);
  }
  {  // the || of :195: iterate(5) runs to mRansacMaxIts = 8; a count equal to minInliers qualifies (>=), its refined count equal
     // to minInliers does not return (>); a tie (10 again) takes no new record; 12 does, refined 11 returns
    Results R({3, 10, 10, 9, 12, 12, 40, 40, 40}, 10, {10, 11, 30});
    EXPECT((R.recHyp == std::vector<int32_t>{1, 4, 6}));
    PnPReplay st = fresh(10, 8);
    const PnPReplay::Step r = R.iterate(&st, 5, &vb);
    EXPECT(r.refined == 1 && r.best < 0 && !r.bNoMore && r.nInliers == 11 && st.mnIterations == 5 && st.mnBestInliers == 12);
    EXPECT(vb.size() == 83 && count_true(vb) == 11 && vb[1] && vb[21] && !vb[23] && !vb[0]);
    // the next call goes on from hypothesis 5: the tie 12 keeps record 1, whose Refine succeeds again at once
    const PnPReplay::Step r2 = R.iterate(&st, 5, &vb);
    EXPECT(r2.refined == 1 && st.mnIterations == 6);
  }
  {  // no Refine succeeds: the tail (:254-267) returns the best hypothesis with bNoMore, after exactly mRansacMaxIts hypotheses
    Results R({3, 10, 10, 9, 12, 12, 11, 5}, 10, {10, 10});
    PnPReplay st = fresh(10, 8);
    const PnPReplay::Step r = R.iterate(&st, 5, &vb);
    EXPECT(r.refined < 0 && r.best == 4 && r.bNoMore && r.nInliers == 12 && st.mnIterations == 8 && count_true(vb) == 12);
    // past mRansacMaxIts a further call runs nIterations more and needs hypotheses that were not supplied
    bool threw = false;
    try { R.iterate(&st, 1, &vb); } catch (const std::out_of_range&) { threw = true; }
    EXPECT(threw);
  }
  {  // nothing qualifies: bNoMore, no pose, vbInliers empty
    Results R({3, 9, 9, 0, 9, 8, 7, 9}, 10, {});
    PnPReplay st = fresh(10, 8);
    const PnPReplay::Step r = R.iterate(&st, 5, &vb);
    EXPECT(r.refined < 0 && r.best < 0 && r.bNoMore && r.nInliers == 0 && vb.empty() && st.mnIterations == 8);
  }
  {  // running out of hypotheses inside the first call
    Results R({3, 9, 9}, 10, {});
    PnPReplay st = fresh(10, 8);
    bool threw = false;
    try { R.iterate(&st, 5, &vb); } catch (const std::out_of_range&) { threw = true; }
    EXPECT(threw && st.mnIterations == 3);
  }
  {  // nIterations above mRansacMaxIts (find() passes mRansacMaxIts itself; here 6 > 4): runs nIterations hypotheses
    Results R({3, 9, 9, 9, 9, 9}, 10, {});
    PnPReplay st = fresh(10, 4);
    const PnPReplay::Step r = R.iterate(&st, 6, &vb);
    EXPECT(r.bNoMore && st.mnIterations == 6);
  }
  return 0;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc >= 4 && !std::strcmp(argv[1], "draws")) {
    const int n = std::atoi(argv[2]), H = std::atoi(argv[3]);
    std::vector<int32_t> draws(4 * (size_t)H), sets(4 * (size_t)H);
    for (int32_t& d : draws)
      if (std::scanf("%d", &d) != 1) return 2;
    if (!pnp_sets_from_draws(n, H, draws.data(), sets.data())) { std::printf("refused\n"); return 0; }
    for (int32_t s : sets) std::printf("%d ", s);
    std::printf("\n");
    return 0;
  }
  if (argc >= 2 && !std::strcmp(argv[1], "params")) {
    int N, mi, mx;
    double prob;
    float eps;
    while (std::scanf("%d %lf %d %d %f", &N, &prob, &mi, &mx, &eps) == 5) {
      orbfe_cpp::PnPReplay st;
      st.N = N;
      st.SetRansacParameters(prob, mi, mx, 4, eps);
      std::printf("%d %d\n", st.mRansacMinInliers, st.mRansacMaxIts);
    }
    return 0;
  }
  if (refusals() || layout_scan_compact() || arithmetic() || replay()) return 1;
  std::printf("ok\n");
  return 0;
}
