// orbfe_pnp_replay.hpp -- the host state of orbfe_cpp::PnPsolver (orbfe_classes.hpp) that needs neither the library nor a
// device: PnPsolver::SetRansacParameters (src/PnPsolver.cc:127-164) with its float and int conversions, and
// PnPsolver::iterate's loop (:178-271) replayed over the two result sets of orbfe_pnp_solve_multi -- the hypotheses and the
// Refine records.  A header of its own so that tests/cpp/pnp_host_san.cpp runs exactly this code under the address and
// undefined-behaviour sanitizers.
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <vector>

namespace orbfe_cpp {

// iterate()'s state: mnIterations and mnBestInliers persist across calls (:69, :198, :225-228)
struct PnPReplay {
  int N = 0;           // correspondences (mvP2D.size())
  int nKeyPoints = 0;  // mvpMapPointMatches.size(): the length of vbInliers
  int mRansacMinInliers = 0, mRansacMaxIts = 0;
  float mRansacEpsilon = 0.0f;
  int mnIterations = 0, mnBestInliers = 0;
  int bestHyp = -1;  // the hypothesis mvbBestInliers / mBestTcw come from, -1: none yet
  int bestRec = -1;  // its Refine record

  // :127-164.  The conversions are the reference's: int nMinInliers = N * (float)epsilon, the two clamps, the (float)
  // division, nIterations = 1 when mRansacMinInliers == N, ceil(log(1 - p) / log(1 - pow(eps, 3))), max(1, min(., maxIts)).
  // Where the reference's quotient is NaN (epsilon > 1: N < minInliers, where iterate() returns at :186 without reading
  // the count) or its conversion to int is undefined, the count is 1 (not finite) or maxIterations (too large).
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                           float epsilon = 0.4f) {
    mRansacEpsilon = epsilon;
    int nMinInliers = (int)((float)N * mRansacEpsilon);  // :141
    if (nMinInliers < minInliers) nMinInliers = minInliers;
    if (nMinInliers < minSet) nMinInliers = minSet;
    mRansacMinInliers = nMinInliers;
    const float ratio = N > 0 ? (float)mRansacMinInliers / (float)N : INFINITY;  // :148 (N = 0: the reference's x / 0)
    if (mRansacEpsilon < ratio) mRansacEpsilon = ratio;
    int nIterations = 1;
    if (mRansacMinInliers != N) {  // :154
      const double q = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)mRansacEpsilon, 3)));  // :157
      if (!std::isfinite(q)) nIterations = 1;
      else if (q >= (double)maxIterations) nIterations = maxIterations;
      else nIterations = (int)q;
    }
    const int m = nIterations < maxIterations ? nIterations : maxIterations;  // :159
    mRansacMaxIts = m > 1 ? m : 1;
  }

  struct Step {
    int refined = -1;  // the Refine record whose pose (mRefinedTcw) iterate() returns, -1: not that return
    int best = -1;     // the hypothesis whose pose (mBestTcw) iterate() returns at :266, -1: not that return
    bool bNoMore = false;
    int nInliers = 0;
  };

  // nIterations as the reference's argument.  Hypothesis h of nHyp has nInliers[h] and its words at words[h * ceil(N / 32) ..];
  // record r of nRec is the Refine problem of hypothesis recHyp[r] (ascending, local to this solver), with recInliers[r] and
  // recWords[r * ceil(N / 32) ..]; correspondence i at bit i & 31 of word i >> 5.  vbInliers [nKeyPoints] is scattered through
  // keyPointIndices [N] (:242-247).  Throws std::out_of_range when the loop needs a hypothesis beyond nHyp.
  Step iterate(int nIterations, int nHyp, const int32_t* nInliers, const uint32_t* words, int nRec, const int32_t* recHyp,
               const int32_t* recInliers, const uint32_t* recWords, const int32_t* keyPointIndices, std::vector<bool>& vbInliers) {
    Step r;
    vbInliers.clear();  // :181
    if (N < mRansacMinInliers) {  // :186
      r.bNoMore = true;
      return r;
    }
    const size_t w = (size_t)((N + 31) / 32);
    auto scatter = [&](const uint32_t* m) {
      vbInliers.assign((size_t)(nKeyPoints > 0 ? nKeyPoints : 0), false);
      for (int i = 0; i < N; i++)
        if ((m[(size_t)(i >> 5)] >> (i & 31)) & 1u) vbInliers[(size_t)keyPointIndices[i]] = true;
    };
    int nCurrentIterations = 0;
    while (mnIterations < mRansacMaxIts || nCurrentIterations < nIterations) {  // :195: || as the reference writes it
      if (mnIterations >= nHyp) throw std::out_of_range("PnPReplay::iterate: out of supplied hypotheses");
      nCurrentIterations++;
      const int h = mnIterations++;
      if (nInliers[h] >= mRansacMinInliers) {  // :222
        if (nInliers[h] > mnBestInliers) {     // :225
          mnBestInliers = nInliers[h];
          bestHyp = h;
          bestRec = -1;
          for (int k = 0; k < nRec; k++)
            if (recHyp[k] == h) bestRec = k;
          if (bestRec < 0) throw std::logic_error("PnPReplay::iterate: the best hypothesis has no Refine record");
        }
        if (recInliers[bestRec] > mRansacMinInliers) {  // Refine() (:307): strictly more
          r.refined = bestRec;
          r.nInliers = recInliers[bestRec];
          scatter(recWords + (size_t)bestRec * w);
          return r;
        }
      }
    }
    if (mnIterations >= mRansacMaxIts) {  // :254
      r.bNoMore = true;
      if (mnBestInliers >= mRansacMinInliers) {
        r.best = bestHyp;
        r.nInliers = mnBestInliers;
        scatter(words + (size_t)bestHyp * w);
      }
    }
    return r;
  }
};

}  // namespace orbfe_cpp
