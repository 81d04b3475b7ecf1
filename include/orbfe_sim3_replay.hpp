// orbfe_sim3_replay.hpp -- the host state of orbfe_cpp::Sim3Solver (orbfe_classes.hpp) that needs neither the library nor a
// device: Sim3Solver::iterate's loop (src/Sim3Solver.cc:150-220) replayed over per-hypothesis results, and the documented
// seeded generator of evaluate_all.  A header of its own so that tests/cpp/sim3_host_san.cpp runs exactly this code under the
// address and undefined-behaviour sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

namespace orbfe_cpp {

// Draw number c (counted over solvers, hypotheses and picks in order, from 0) of evaluate_all(solvers, seed): splitmix64's
// output for the state seed + (c + 1) * 0x9E3779B97F4A7C15 (mod 2^64), reduced modulo `size`, the length n - i of the list the
// draw indexes.  Not the reference's rand() stream.
inline int32_t sim3_seeded_draw(uint64_t seed, uint64_t c, int size) {
  uint64_t z = seed + (c + 1) * 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  z = z ^ (z >> 31);
  return (int32_t)(z % (uint64_t)size);
}

// iterate()'s state: mnIterations and mnBestInliers persist across calls (:38, :141, :195-198)
struct Sim3Replay {
  int N = 0, mN1 = 0, mRansacMinInliers = 0, mRansacMaxIts = 0;
  int mnIterations = 0, mnBestInliers = 0;

  struct Step {
    int accepted = -1;  // the hypothesis iterate() returns, -1: an empty cv::Mat
    int best = -1;      // the last hypothesis THIS call took as the best so far (:195-202), -1: none.  An index into the list
                        // this call was given: whoever keeps the best estimate copies it now, as the reference clones
                        // mBestT12, since the list may be another one at the next call
    bool bNoMore = false;
    int nInliers = 0;
  };

  // nIterations more hypotheses of nInliers[0 .. mRansacMaxIts); the words of hypothesis h are
  // words[h * ceil(N / 32) ..], pair i at bit i & 31 of word i >> 5; vbInliers [mN1] is scattered through indices1 [N]
  Step iterate(int nIterations, const int32_t* nInliers, const uint32_t* words, const int32_t* indices1,
               std::vector<bool>& vbInliers) {
    Step r;
    vbInliers.assign((size_t)(mN1 > 0 ? mN1 : 0), false);  // :153
    if (N < mRansacMinInliers) {                           // :156
      r.bNoMore = true;
      return r;
    }
    const size_t w = (size_t)((N + 31) / 32);
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts && nCurrentIterations < nIterations) {  // :168
      nCurrentIterations++;
      const int h = mnIterations++;
      if (nInliers[h] >= mnBestInliers) {  // :195
        mnBestInliers = nInliers[h];
        r.best = h;
        if (nInliers[h] > mRansacMinInliers) {  // :204
          r.accepted = h;
          r.nInliers = nInliers[h];
          for (int i = 0; i < N; i++)  // :207-209
            if ((words[(size_t)h * w + (size_t)(i >> 5)] >> (i & 31)) & 1u) vbInliers[(size_t)indices1[i]] = true;
          return r;
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) r.bNoMore = true;  // :216
    return r;
  }
};

}  // namespace orbfe_cpp
