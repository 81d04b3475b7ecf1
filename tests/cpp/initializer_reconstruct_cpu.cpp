// Stand-alone CPU build of csrc/initializer_reconstruct_math.h -- the arithmetic k_init_reconstruct.hip compiles -- on one scene
// file of tests/initializer_reconstruct_ref.py: runs every hypothesis of every problem through recon_hypothesis_host (the
// layout from csrc/initializer_host.h) and writes the result file.  Build with -ffp-contract=off.
//   initializer_reconstruct_cpu scene.txt out.txt [repeat]     repeat > 0: also prints the seconds of one pass (the median is
//                                                              the caller's), for tools/initializer_reconstruct_latency.py
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "initializer_host.h"
#include "initializer_reconstruct_scene.h"

using namespace orbfe;

static void run_all(const std::vector<ReconProblem>& probs, const std::vector<int32_t>& hypProb, ReconOperands& o) {
  for (size_t g = 0; g < o.G; g++) {
    const size_t k = (size_t)hypProb[g];
    const ReconProblem& P = probs[k];
    const int hi = (int)g - P.hyp0;
    const size_t slot = (size_t)P.slot0 + (size_t)hi * (size_t)P.nPairs;
    std::vector<uint64_t> keys((size_t)P.nPairs + 1);
    uint8_t status;
    bool deg;
    int32_t nInl;
    recon_hypothesis_host(P, o.pairs.data() + 4 * (size_t)P.pair0, o.words.data() + P.word0, hi, &o.R[9 * g], &o.t[3 * g], &o.nGood[g],
                          &o.cosSel[g], &status, o.x3d.data() + 3 * slot, o.pairFlags.data() + slot, keys.data(), &deg, &nInl);
    o.hypStatus[g] = status;
    if (hi == 0) {
      o.nInliers[k] = nInl;
      o.problemStatus[k] = (uint8_t)(deg ? kReconDegenerate : kReconProblemOk);
    }
  }
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  ReconScene sc;
  if (!recon_read_scene(argv[1], &sc)) { std::fprintf(stderr, "cannot read %s\n", argv[1]); return 2; }
  ReconOperands o(sc);
  const int K = sc.K;
  if (const char* e = recon_check(K, o.pairOff.back(), o.wordOff.back(), o.pairOff.data(), o.pairs.data(), o.kind.data(), o.model.data(),
                                  o.K4.data(), o.sigma.data(), o.words.data(), o.wordOff.data(), o.hypOff.data(), o.slotOff.data(),
                                  o.R.data(), o.t.data(), o.nGood.data(), o.cosSel.data(), o.hypStatus.data(), o.x3d.data(),
                                  o.pairFlags.data(), o.problemStatus.data(), o.nInliers.data())) {
    // (empty vectors have NULL data: a scene whose arrays are empty is refused like any NULL array)
    std::fprintf(stderr, "refused: %s\n", e);
    return 3;
  }
  std::vector<ReconProblem> probs;
  std::vector<int32_t> hypProb;
  recon_layout(K, o.pairOff.data(), o.kind.data(), o.model.data(), o.K4.data(), o.sigma.data(), o.wordOff.data(), o.hypOff.data(),
               o.slotOff.data(), &probs, &hypProb);
  run_all(probs, hypProb, o);
  const int repeat = argc > 3 ? std::atoi(argv[3]) : 0;
  for (int i = 0; i < repeat; i++) {
    const auto t0 = std::chrono::steady_clock::now();
    run_all(probs, hypProb, o);
    std::printf("%.9f\n", std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count());
  }
  return recon_write_result(argv[2], o) ? 0 : 1;
}
