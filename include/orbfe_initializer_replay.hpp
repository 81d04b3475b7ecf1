// orbfe_initializer_replay.hpp -- the host side of orbfe_cpp::Initializer (orbfe_classes.hpp) that needs neither the library
// nor a device: the scans of FindHomography / FindFundamental over per-hypothesis scores (src/Initializer.cc:174-198,
// :229-254) and the choice between the models (:124-131).  A header of its own so that tests/cpp/initializer_host_san.cpp
// runs exactly this code under the address and undefined-behaviour sanitizers.
#pragma once
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
};

}  // namespace orbfe_cpp
