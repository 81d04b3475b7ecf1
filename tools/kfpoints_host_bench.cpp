// The CPU yardstick of tools/kfpoints_latency.py: the compiled host loops of csrc/obsgraph_host.h (kfpoints_union_flat,
// kfpoints_tracked_flat -- the reference's own loops over flat arrays) on one thread, over the arrays the device call was
// given.  Built without sanitizers.  Reads one int32 file:
//   P K W nCases reps | rows [K][W] | len [K] | bad [P] | nObs [P] | per case: kind (0 union, 1 tracked) nQueries minObs
//   offsets [nQueries + 1] kfs [offsets[nQueries]]
// and prints per case "case <i> <median ms> <count of query 0> <sum of all counts>".
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <vector>

#include "obsgraph_host.h"

using namespace orbfe;

static volatile int32_t sink;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> in;
  int32_t buf[4096];
  size_t got;
  while ((got = std::fread(buf, 4, 4096, f)) > 0) in.insert(in.end(), buf, buf + got);
  std::fclose(f);
  size_t at = 0;
  const int P = in[at++], K = in[at++], W = in[at++], nCases = in[at++], reps = in[at++];
  const int32_t* rows = &in[at]; at += (size_t)K * W;
  const int32_t* len = &in[at]; at += (size_t)K;
  std::vector<ObsPointMeta> meta((size_t)P);
  for (int p = 0; p < P; p++) meta[(size_t)p] = ObsPointMeta{0, in[at + (size_t)P + p], in[at + p], -1};
  at += 2 * (size_t)P;
  std::vector<int32_t> stamp((size_t)P, 0), out((size_t)P);
  int32_t mark = 0;
  for (int c = 0; c < nCases; c++) {
    const int kind = in[at++], Q = in[at++], minObs = in[at++];
    const int32_t* off = &in[at]; at += (size_t)Q + 1;
    const int32_t* kfs = &in[at]; at += (size_t)off[Q];
    std::vector<double> ms;
    long long first = 0, sum = 0;
    for (int r = 0; r < reps + 1; r++) {  // the first pass warms the caches and is dropped
      const auto t0 = std::chrono::steady_clock::now();
      first = sum = 0;
      for (int q = 0; q < Q; q++) {
        int n = 0;
        if (kind == 0) {
          n = kfpoints_union_flat(rows, len, W, meta.data(), off[q + 1] - off[q], kfs + off[q], stamp.data(), ++mark, out.data(), P);
          sink = out[(size_t)(n > 0 ? n - 1 : 0)];  // the list is read: its stores cannot be dropped
        } else {
          const int k = kfs[off[q]];
          n = kfpoints_tracked_flat(rows + (size_t)k * W, len[k], meta.data(), minObs);
        }
        if (q == 0) first = n;
        sum += n;
      }
      const auto t1 = std::chrono::steady_clock::now();
      if (r) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    std::printf("case %d %.4f %lld %lld\n", c, ms[ms.size() / 2], first, sum);
  }
  return 0;
}
