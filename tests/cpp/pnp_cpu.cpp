// Stand-alone program: the arithmetic of csrc/pnp_math.h -- the very code k_pnp.hip compiles for the device -- and the checks,
// layout and record scan of csrc/pnp_host.h on the CPU: every hypothesis, the scan, every Refine record, with all sums formed
// point by point in index order.  Reads a scene file (tests/pnp_ref.py: write_scene), writes per hypothesis and per record
// "n_inliers status pose[12] words..", prints the single-thread time.  Build with -ffp-contract=off.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pnp_host.h"

using namespace orbfe;

namespace {

struct ListPoints {  // correspondences idx[0 .. n) of a candidate
  const float* p3d;
  const float* p2d;
  const int32_t* idx;
  int point0, count;
  int n() const { return count; }
  void get(int i, double pw[3], double uv[2]) const {
    const size_t p = (size_t)(point0 + idx[i]);
    pw[0] = p3d[3 * p]; pw[1] = p3d[3 * p + 1]; pw[2] = p3d[3 * p + 2];
    uv[0] = p2d[2 * p]; uv[1] = p2d[2 * p + 1];
  }
};

struct Out {
  std::vector<int32_t> nInliers;
  std::vector<uint8_t> status;
  std::vector<float> pose;
  std::vector<uint32_t> words;
  std::vector<int32_t> wordOff;
};

void solve(const PnpCandidate& C, const ListPoints& P, const std::vector<float>& p3d, const std::vector<float>& p2d,
           const std::vector<float>& maxErr, int item, Out* o) {
  PnpWork W;
  double R[9], t[3];
  pnp_compute_pose(P, C.K, &W, R, t);
  const bool bad = pnp_nonfinite(R, t);
  uint32_t* w = o->words.data() + C.word0 + (size_t)(item - C.hyp0) * C.words;
  for (int i = 0; i < C.words; i++) w[i] = 0;
  int count = 0;
  for (int i = 0; i < C.nPoints && !bad; i++) {
    const size_t p = (size_t)(C.point0 + i);
    if (pnp_is_inlier(R, t, C.K, &p3d[3 * p], &p2d[2 * p], maxErr[p])) { w[i >> 5] |= 1u << (i & 31); count++; }
  }
  o->nInliers[item] = count;
  o->status[item] = (uint8_t)(bad ? kPnpNonfinite : kPnpOk);
  for (int i = 0; i < 9; i++) o->pose[12 * (size_t)item + i] = (float)R[i];
  for (int i = 0; i < 3; i++) o->pose[12 * (size_t)item + 9 + i] = (float)t[i];
}

void alloc(Out* o, int K, int I, const std::vector<int32_t>& pointOff, const std::vector<int32_t>& itemOff) {
  size_t W = 0;
  for (int k = 0; k < K; k++) W += (size_t)(itemOff[k + 1] - itemOff[k]) * (size_t)((pointOff[k + 1] - pointOff[k] + 31) / 32);
  o->nInliers.assign((size_t)I, 0); o->status.assign((size_t)I, 0); o->pose.assign((size_t)I * 12, 0.f);
  o->words.assign(W ? W : 1, 0); o->wordOff.assign((size_t)K + 1, 0);
}

void write(FILE* f, const Out& o, const std::vector<PnpCandidate>& cands, const std::vector<int32_t>& itemCand) {
  for (size_t h = 0; h < itemCand.size(); h++) {
    const PnpCandidate& C = cands[itemCand[h]];
    std::fprintf(f, "%d %d", o.nInliers[h], (int)o.status[h]);
    for (int i = 0; i < 12; i++) std::fprintf(f, " %.9g", (double)o.pose[12 * h + i]);
    for (int i = 0; i < C.words; i++) std::fprintf(f, " %u", o.words[C.word0 + ((int)h - C.hyp0) * (size_t)C.words + i]);
    std::fprintf(f, "\n");
  }
}

}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) { std::printf("usage: pnp_cpu scene result [repeats]\n"); return 2; }
  const int repeats = argc > 3 ? std::atoi(argv[3]) : 1;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) { std::printf("cannot read %s\n", argv[1]); return 2; }
  int K = 0;
  if (std::fscanf(f, "%d", &K) != 1 || K < 0) return 2;
  std::vector<int32_t> pointOff(1, 0), hypOff(1, 0), sets, minInl;
  std::vector<float> p3d, p2d, maxErr, cam;
  for (int k = 0; k < K; k++) {
    int n, H, mi;
    float c[4];
    if (std::fscanf(f, "%d %d %d %f %f %f %f", &n, &H, &mi, c, c + 1, c + 2, c + 3) != 7) return 2;
    cam.insert(cam.end(), c, c + 4);
    minInl.push_back(mi);
    for (int i = 0; i < n; i++) {
      float v[6];
      if (std::fscanf(f, "%f %f %f %f %f %f", v, v + 1, v + 2, v + 3, v + 4, v + 5) != 6) return 2;
      p3d.insert(p3d.end(), v, v + 3); p2d.insert(p2d.end(), v + 3, v + 5); maxErr.push_back(v[5]);
    }
    for (int i = 0; i < 4 * H; i++) {
      int s;
      if (std::fscanf(f, "%d", &s) != 1) return 2;
      sets.push_back(s);
    }
    pointOff.push_back(pointOff.back() + n);
    hypOff.push_back(hypOff.back() + H);
  }
  std::fclose(f);
  const int N = pointOff.back(), H = hypOff.back();
  Out oh, orr;
  alloc(&oh, K, H, pointOff, hypOff);
  const char* e = pnp_check_common(K, N, H, pointOff.data(), p3d.data(), p2d.data(), maxErr.data(), cam.data(), hypOff.data(),
                                   sets.data(), oh.nInliers.data(), oh.status.data(), oh.pose.data(), oh.wordOff.data(),
                                   oh.words.data());
  if (!e && H > 0) e = pnp_check_sets(K, pointOff.data(), hypOff.data(), sets.data());
  if (e) { std::printf("refused: %s\n", e); return 1; }
  std::vector<PnpCandidate> cands, rcands;
  std::vector<int32_t> hypCand, recCand, recHyp, recOff((size_t)K + 1), idxOff, idx;
  double bestUs = 1e300;
  for (int rep = 0; rep < (repeats > 0 ? repeats : 1); rep++) {
    const auto t0 = std::chrono::steady_clock::now();
    pnp_layout(K, pointOff.data(), hypOff.data(), cam.data(), oh.wordOff.data(), &cands, &hypCand);
    for (int h = 0; h < H; h++) {
      const PnpCandidate& C = cands[hypCand[h]];
      const ListPoints P = {p3d.data(), p2d.data(), sets.data() + 4 * (size_t)h, C.point0, 4};
      solve(C, P, p3d, p2d, maxErr, h, &oh);
    }
    pnp_scan_records(K, hypOff.data(), oh.nInliers.data(), minInl.data(), recOff.data(), &recHyp);
    std::vector<uint32_t> masks;
    for (int k = 0; k < K; k++)
      for (int r = recOff[k]; r < recOff[k + 1]; r++) {
        const uint32_t* w = oh.words.data() + cands[k].word0 + (size_t)(recHyp[r] - hypOff[k]) * cands[k].words;
        masks.insert(masks.end(), w, w + cands[k].words);
      }
    const int R = (int)recHyp.size();
    alloc(&orr, K, R, pointOff, recOff);
    if (R > 0 && (e = pnp_check_masks(K, pointOff.data(), recOff.data(), masks.data()))) { std::printf("refused: %s\n", e); return 1; }
    pnp_layout(K, pointOff.data(), recOff.data(), cam.data(), orr.wordOff.data(), &rcands, &recCand);
    pnp_compact(K, pointOff.data(), recOff.data(), masks.data(), &idxOff, &idx);
    for (int r = 0; r < R; r++) {
      const PnpCandidate& C = rcands[recCand[r]];
      const ListPoints P = {p3d.data(), p2d.data(), idx.data() + idxOff[r], C.point0, idxOff[r + 1] - idxOff[r]};
      solve(C, P, p3d, p2d, maxErr, r, &orr);
    }
    const double us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
    if (us < bestUs) bestUs = us;
  }
  FILE* g = std::fopen(argv[2], "w");
  if (!g) return 2;
  std::fprintf(g, "%d %d\n", H, (int)recHyp.size());
  write(g, oh, cands, hypCand);
  for (int k = 0; k <= K; k++) std::fprintf(g, "%d ", recOff[k]);
  std::fprintf(g, "\n");
  for (int32_t h : recHyp) std::fprintf(g, "%d ", h);
  std::fprintf(g, "\n");
  write(g, orr, rcands, recCand);
  std::fclose(g);
  std::printf("hypotheses=%d records=%d cpu_us=%.1f\n", H, (int)recHyp.size(), bestUs);
  return 0;
}
