// orbfe_cpp::Sim3Solver (include/orbfe_classes.hpp) on one scene file written by tests/test_gpu_sim3_cpp.py
// (tests/sim3_ref.py: write_scene): SetRansacParameters(0.99, minInliers, 300) as src/LoopClosing.cc:328, evaluate_all with the
// scene's triples, then the caller's round-robin of iterate(5) (src/LoopClosing.cc:342-404, going on after an acceptance).
// Prints one line per iterate call for the Python test to compare with the restatement's state machine.
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "orbfe_classes.hpp"
#include "sim3_scene.h"

int main(int argc, char** argv) {
  using namespace orbfe_cpp;
  if (argc < 3) return 2;
  const int minInliers = std::atoi(argv[2]);
  Sim3Scene S;
  if (!sim3_read_scene(argv[1], &S)) { std::printf("error=cannot_read_scene\n"); return 2; }
  try {
    std::vector<std::unique_ptr<Sim3Solver>> own;
    std::vector<Sim3Solver*> solvers;
    std::vector<std::vector<int32_t>> triples;
    for (const Sim3SceneCandidate& c : S.cands) {
      own.emplace_back(new Sim3Solver(c.indices1, c.x1, c.x2, c.sigma2_1, c.sigma2_2, c.cam1, c.cam2, c.N1, S.fixScale != 0));
      own.back()->SetRansacParameters(0.99, minInliers, 300);
      solvers.push_back(own.back().get());
      triples.push_back(c.triples);
      std::printf("solver %d hypotheses %d\n", (int)solvers.size() - 1, own.back()->nHypotheses());
    }
    bool threw = false;
    try {
      bool b; std::vector<bool> v; int n; float T[16];
      solvers[0]->iterate(5, b, v, n, T);
    } catch (const std::logic_error&) { threw = true; }
    std::printf("iterate_before_evaluate_throws %d\n", (int)threw);
    threw = false;
    try { solvers[1]->GetEstimatedScale(); } catch (const std::logic_error&) { threw = true; }
    std::printf("estimate_before_any_hypothesis_throws %d\n", (int)threw);
    // the documented generator, for the Python test to compare with loop_closing.seeded_draws
    std::printf("draws");
    for (uint64_t c = 0; c < 12; c++) std::printf(" %d", sim3_seeded_draw(7, 100 + c, 80 - (int)(c % 3)));
    std::printf(" %d %d\n", sim3_seeded_draw(0xFFFFFFFFFFFFFFFFull, 0, 1000003), sim3_seeded_draw(0, 0, 3));
    Sim3Solver::evaluate_all(solvers, triples);
    std::vector<bool> discarded(solvers.size(), false);
    for (int round = 0, left = (int)solvers.size(); left > 0 && round < 200; round++)
      for (size_t k = 0; k < solvers.size(); k++) {
        if (discarded[k]) continue;
        bool bNoMore = false;
        std::vector<bool> vb;
        int nInliers = 0;
        float T12[16];
        const bool ok = solvers[k]->iterate(5, bNoMore, vb, nInliers, T12);
        long sum = 0;
        int cnt = 0;
        for (size_t i = 0; i < vb.size(); i++)
          if (vb[i]) { sum += (long)i; cnt++; }
        std::printf("call %zu %d %d %d %d %ld %d %d", k, (int)ok, (int)bNoMore, nInliers, cnt, sum, solvers[k]->iterations(), solvers[k]->bestInliers());
        if (ok) {
          float R[9], t[3];
          solvers[k]->GetEstimatedRotation(R); solvers[k]->GetEstimatedTranslation(t);
          bool same = T12[15] == 1.0f;
          for (int i = 0; i < 3; i++) {
            same = same && T12[4 * i + 3] == t[i];
            for (int j = 0; j < 3; j++) same = same && T12[4 * i + j] == solvers[k]->GetEstimatedScale() * R[3 * i + j];
          }
          std::printf(" %d", (int)same);
          for (int i = 0; i < 12; i++) std::printf(" %.9g", T12[i]);
        }
        std::printf("\n");
        if (bNoMore) { discarded[k] = true; left--; }
      }
    // a seed in place of triples: the same seed draws the same, valid triples.  SetRansacParameters starts the iterations anew
    // (:141); mnBestInliers stays, as in the reference, so find() returns the first hypothesis that reaches the best count again
    solvers[1]->SetRansacParameters(0.99, minInliers, 300);
    Sim3Solver::evaluate_all(solvers, (uint64_t)7);
    std::vector<bool> vb;
    int n1 = 0, n2 = 0;
    float Ta[16], Tb[16];
    const bool a = solvers[1]->find(vb, n1, Ta);
    solvers[1]->SetRansacParameters(0.99, minInliers, 300);
    Sim3Solver::evaluate_all(solvers, (uint64_t)7);
    const bool b = solvers[1]->find(vb, n2, Tb);
    std::printf("seeded %d %d %d\n", (int)a, (int)b, (int)(a && b && n1 == n2 && !std::memcmp(Ta, Tb, sizeof Ta)));
    // re-parameterised to FEWER hypotheses after use: the estimate of the best hypothesis taken so far stays what it was (the
    // reference keeps mBestRotation / mBestTranslation / mBestScale across SetRansacParameters) until a new best is taken
    float R0[9], t0[3], R1[9], t1[3];
    solvers[1]->GetEstimatedRotation(R0); solvers[1]->GetEstimatedTranslation(t0);
    const float s0 = solvers[1]->GetEstimatedScale();
    solvers[1]->SetRansacParameters(0.99, minInliers, 2);
    std::vector<std::vector<int32_t>> few(triples);
    few[1].assign({3, 0, 1, 5, 2, 4});  // (pairs 3 and 5 of the class scene's good candidate are outliers: neither is a new best)
    few[0].resize(3 * (size_t)solvers[0]->nHypotheses());
    Sim3Solver::evaluate_all(solvers, few);
    solvers[1]->GetEstimatedRotation(R1); solvers[1]->GetEstimatedTranslation(t1);
    bool kept = solvers[1]->nHypotheses() == 2 && s0 == solvers[1]->GetEstimatedScale() && !std::memcmp(R0, R1, sizeof R0) && !std::memcmp(t0, t1, sizeof t0);
    bool bNoMore = false;
    int nIn = 0;
    const bool took = solvers[1]->iterate(5, bNoMore, vb, nIn, Ta);
    solvers[1]->GetEstimatedRotation(R1);
    kept = kept && bNoMore && solvers[1]->iterations() == 2 && (took || !std::memcmp(R0, R1, sizeof R0));
    solvers[1]->SetRansacParameters(0.99, 1000, 300);  // minInliers above N: no hypotheses
    Sim3Solver::evaluate_all(solvers, std::vector<std::vector<int32_t>>{few[0], {}, {}});
    const bool none = !solvers[1]->iterate(5, bNoMore, vb, nIn, Ta) && bNoMore && solvers[1]->nHypotheses() == 0;
    solvers[1]->GetEstimatedRotation(R1);
    std::printf("reparameterised %d %d %d\n", (int)kept, (int)none, (int)(took || !std::memcmp(R0, R1, sizeof R0)));
  } catch (const std::exception& e) {
    std::printf("error=%s\n", e.what());
    return 1;
  }
  return 0;
}
