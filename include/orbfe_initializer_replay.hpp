// orbfe_initializer_replay.hpp -- the host side of orbfe_cpp::Initializer (orbfe_classes.hpp) that needs neither the library
// nor a device: the scans of FindHomography / FindFundamental over per-hypothesis scores (src/Initializer.cc:174-198,
// :229-254), the choice between the models (:124-131) and the tails of ReconstructF / ReconstructH (:568-641, :778-823) over
// the per-hypothesis results of orbfe_initializer_reconstruct.  A header of its own so that tests/cpp/initializer_host_san.cpp
// and tests/cpp/initializer_reconstruct_host_san.cpp run exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orbfe_cpp {

struct InitializerReplay {
  // what FindHomography / FindFundamental leave: the FIRST hypothesis whose score is strictly greater than the best so far,
  // which starts at 0.0 (:154, :192).  NaN > x is false, so a hypothesis with a NaN score is never taken.  best = -1: no
  // hypothesis scored above 0 -- the model stays empty and the mask all-false, as in the reference.
  struct Pick {
    int best = -1;
    double score = 0.0;
  };
  // score [H * 2], the layout of orbfe_initializer_ransac: entry 2 h + model
  static Pick scan(int H, int model, const double* score) {
    Pick p;
    for (int h = 0; h < H; h++) {
      const double currentScore = score[2 * (size_t)h + (size_t)model];
      if (currentScore > p.score) {  // :192, :248
        p.best = h;
        p.score = currentScore;
      }
    }
    return p;
  }
  // :124: RH = SH / (SH + SF); 0 / 0 is NaN, for which RH > 0.40 is false as in the reference
  static double ratio(double SH, double SF) { return SH / (SH + SF); }
  static bool choose_h(double RH) { return RH > 0.40; }  // :127
  // vbMatchesInliers [n] of hypothesis `best` of `model`: words = the problem's mask words, pair i at bit i & 31 of word
  // i >> 5 of the words of (best, model)
  static void inliers(int n, int best, int model, const uint32_t* words, std::vector<bool>& vb) {
    vb.assign((size_t)(n > 0 ? n : 0), false);  // :155, :219
    if (best < 0) return;
    const size_t w = (size_t)((n + 31) / 32);
    const uint32_t* m = words + (2 * (size_t)best + (size_t)model) * w;
    for (int i = 0; i < n; i++) vb[(size_t)i] = ((m[i >> 5] >> (i & 31)) & 1u) != 0;
  }

  // ---- the tails of ReconstructF / ReconstructH over the per-hypothesis results of orbfe_initializer_reconstruct ----
  // CheckRT's parallax (:1018-1026): acos of the selected cosine in degrees, 0 when nGood == 0.  The device returns the
  // cosine; the one acos is taken here.
  static double parallax_degrees(int nGood, double cosSel) { return nGood > 0 ? std::acos(cosSel) * 180.0 / 3.14159265358979323846 : 0.0; }
  struct Outcome {
    bool success = false;
    int best = -1;  // the hypothesis whose R, t, points and flags are returned; -1 when not successful
  };
  // :568-641.  N = the number of inliers (:540-543); nGood, parallax [4]
  static Outcome reconstruct_f(int N, const int* nGood, const double* parallax, double minParallax = 1.0, int minTriangulated = 50) {
    Outcome o;
    int maxGood = nGood[0];
    for (int i = 1; i < 4; i++) maxGood = nGood[i] > maxGood ? nGood[i] : maxGood;  // :568
    const int nMinGood = static_cast<int>(0.9 * N) > minTriangulated ? static_cast<int>(0.9 * N) : minTriangulated;  // :575
    int nsimilar = 0;
    for (int i = 0; i < 4; i++)
      if (nGood[i] > 0.7 * maxGood) nsimilar++;  // :578-585
    if (maxGood < nMinGood || nsimilar > 1) return o;  // :589
    for (int i = 0; i < 4; i++)  // :595-639: the `if / else if` chain enters the FIRST hypothesis that equals maxGood only
      if (maxGood == nGood[i]) {
        if (parallax[i] > minParallax) { o.success = true; o.best = i; }
        return o;
      }
    return o;
  }
  // :778-823.  nGood, parallax [8]
  static Outcome reconstruct_h(int N, const int* nGood, const double* parallax, double minParallax = 1.0, int minTriangulated = 50) {
    Outcome o;
    int bestGood = 0, secondBestGood = 0, bestSolutionIdx = -1;
    double bestParallax = -1.0;
    for (int i = 0; i < 8; i++) {
      if (nGood[i] > bestGood) {  // :797
        secondBestGood = bestGood;
        bestGood = nGood[i];
        bestSolutionIdx = i;
        bestParallax = parallax[i];
      } else if (nGood[i] > secondBestGood) {  // :806
        secondBestGood = nGood[i];
      }
    }
    if (secondBestGood < 0.75 * bestGood && bestParallax >= minParallax && bestGood > minTriangulated && bestGood > 0.9 * N) {  // :813
      o.success = true;
      o.best = bestSolutionIdx;
    }
    return o;
  }
  // bool [n] -> its ceil(n / 32) mask words (the input format of orbfe_initializer_reconstruct)
  static void pack(const std::vector<bool>& vb, std::vector<uint32_t>& words) {
    words.assign((vb.size() + 31) / 32, 0u);
    for (size_t i = 0; i < vb.size(); i++)
      if (vb[i]) words[i >> 5] |= 1u << (i & 31);
  }
};

}  // namespace orbfe_cpp
