// orbfe_cpp::Optimizer::LocalBundleAdjustment / BundleAdjustment (include/orbfe_classes.hpp) on one scene the Python test
// writes (tests/lba_check.py: write_scene): runs the class form, compares it with the C-ABI call bit for bit, and writes the
// class form's results in the layout of read_result for tests/test_gpu_lba_cpp.py to compare with the Python binding's.
// usage: test_lba scene results.  Prints key=value tokens.
#include <cstdio>
#include <cstring>
#include <vector>

#include "orbfe_classes.hpp"

namespace {
template <typename T>
bool rd(std::FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
bool wr(std::FILE* f, const T* p, size_t n) { return n == 0 || std::fwrite(p, sizeof(T), n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[9];
  if (std::fread(hd, 4, 9, f) != 9) return 2;
  const int nLocal = hd[0], nFixed = hd[1], nPoints = hd[2], nEdges = hd[3], hasFixed = hd[4], global = hd[5], nIt = hd[6], robust = hd[7];
  const size_t nT = (size_t)nLocal + nFixed, nE = (size_t)nEdges;
  orbfe_cpp::Optimizer::BundleGraph g;
  g.nLocal = nLocal;
  std::vector<uint8_t> flags;
  if (!rd(f, g.Tcw, 16 * nT) || !rd(f, flags, (size_t)nLocal) || !rd(f, g.cam, 5 * nT) || !rd(f, g.Xw, 3 * (size_t)nPoints) ||
      !rd(f, g.edgePose, nE) || !rd(f, g.edgePoint, nE) || !rd(f, g.u, nE) || !rd(f, g.v, nE) || !rd(f, g.uRight, nE) || !rd(f, g.invSigma2, nE))
    return 2;
  std::fclose(f);
  if (hasFixed) g.localIsFixed = flags;

  std::vector<double> T, X, T2(16 * (size_t)nLocal), X2(3 * (size_t)nPoints), chi2(nE);
  std::vector<uint8_t> erase(nE, 0), erase2(nE, 0), level1(nE, 0);
  orbfe_lba_stats st{}, st2{};
  int rc;
  if (global) {
    orbfe_cpp::Optimizer::BundleAdjustment(g, T, X, nIt, nullptr, robust != 0, &st);
    rc = orbfe_bundle_adjustment(0, nLocal, nFixed, g.Tcw.data(), hasFixed ? flags.data() : nullptr, g.cam.data(), nPoints, g.Xw.data(),
                                 nEdges, g.edgePose.data(), g.edgePoint.data(), g.u.data(), g.v.data(), g.uRight.data(), g.invSigma2.data(),
                                 nIt, robust, nullptr, T2.data(), X2.data(), &st2, chi2.data());
  } else {
    erase = orbfe_cpp::Optimizer::LocalBundleAdjustment(g, T, X, nullptr, &st);
    rc = orbfe_local_bundle_adjustment(0, nLocal, nFixed, g.Tcw.data(), hasFixed ? flags.data() : nullptr, g.cam.data(), nPoints,
                                       g.Xw.data(), nEdges, g.edgePose.data(), g.edgePoint.data(), g.u.data(), g.v.data(), g.uRight.data(),
                                       g.invSigma2.data(), nullptr, T2.data(), X2.data(), erase2.data(), level1.data(), &st2, chi2.data());
  }
  const bool equal = rc == ORBFE_OK && T.size() == T2.size() && X.size() == X2.size() &&
                     std::memcmp(T.data(), T2.data(), T.size() * sizeof(double)) == 0 &&
                     std::memcmp(X.data(), X2.data(), X.size() * sizeof(double)) == 0 && erase == erase2 &&
                     std::memcmp(&st, &st2, sizeof st) == 0;
  // the stop flag at entry: nothing optimised
  volatile int stop = 1;
  std::vector<double> Ts, Xs;
  orbfe_lba_stats sts{};
  bool stopped = true;
  if (!global) {
    const std::vector<uint8_t> es = orbfe_cpp::Optimizer::LocalBundleAdjustment(g, Ts, Xs, &stop, &sts);
    stopped = sts.stopped == 1 && sts.rounds == 0;
    for (uint8_t b : es) stopped = stopped && b == 0;
    for (size_t i = 0; i < Xs.size(); i++) stopped = stopped && Xs[i] == (double)g.Xw[i];
  }
  int threw = 0;
  try {
    orbfe_cpp::Optimizer::BundleGraph b = g;
    b.u.pop_back();
    orbfe_cpp::Optimizer::LocalBundleAdjustment(b, Ts, Xs);
  } catch (const std::invalid_argument&) { threw++; }
  try {
    orbfe_cpp::Optimizer::BundleGraph b = g;
    b.cam.pop_back();
    orbfe_cpp::Optimizer::BundleAdjustment(b, Ts, Xs);
  } catch (const std::invalid_argument&) { threw++; }
  try {  // what the library refuses arrives as an exception
    orbfe_cpp::Optimizer::BundleGraph b = g;
    b.edgePoint[0] = nPoints;
    orbfe_cpp::Optimizer::LocalBundleAdjustment(b, Ts, Xs);
  } catch (const std::exception&) { threw++; }

  std::FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 2;
  const int32_t ints[8] = {st.rounds, st.stopped, st.iterations[0], st.iterations[1], st.trials[0], st.trials[1], st.termination[0], st.termination[1]};
  bool ok = wr(o, T.data(), T.size()) && wr(o, X.data(), X.size()) && wr(o, erase.data(), nE) && wr(o, level1.data(), nE) &&
            wr(o, chi2.data(), nE) && wr(o, ints, 8) && wr(o, st.lambda, 2) && wr(o, st.chi2, 2);
  ok = std::fclose(o) == 0 && ok;
  if (!ok) return 2;
  std::printf("class_equal=%d stopped=%d threw=%d rounds=%d\n", equal ? 1 : 0, stopped ? 1 : 0, threw, st.rounds);
  return 0;
}
