// The host steps a caller of the array form (orbfe_distinctive_descriptors) has around the device call, compiled (-O2, one
// thread) so that tools/distinctive_latency.py measures them as a C++ caller would pay them, over flat arrays instead of
// the reference's MapPoint / KeyFrame objects (a pointer walk would only be slower): the rows as a CSR of (kf, idx) in
// ascending mnId, the bad flags, and the key frames' descriptors as uint8 [kf][width][32].
#include <cstdint>
#include <cstring>

extern "C" {

// MapPoint::ComputeDistinctiveDescriptors :288-294 for slot[n]: the descriptors of the entries whose key frame is not bad,
// in row order, into out_desc; out_off[n + 1].  Returns the number of descriptors.
int distinctive_gather(int n, const int32_t* slot, const int32_t* row_off, const int32_t* row_kf, const uint16_t* row_idx,
                       const uint8_t* kf_bad, const uint8_t* kf_desc, int width, uint8_t* out_desc, int32_t* out_off) {
  int32_t at = 0;
  out_off[0] = 0;
  for (int i = 0; i < n; i++) {
    for (int32_t e = row_off[slot[i]]; e < row_off[slot[i] + 1]; e++) {
      if (kf_bad[row_kf[e]]) continue;
      std::memcpy(out_desc + (size_t)at * 32, kf_desc + ((size_t)row_kf[e] * (size_t)width + row_idx[e]) * 32, 32);
      at++;
    }
    out_off[i + 1] = at;
  }
  return at;
}

// :332 for slot[n]: winners[i] = the best[i]-th descriptor of list i (left alone where the list is empty)
void distinctive_pick(int n, const int32_t* best, const uint8_t* lists, const int32_t* off, uint8_t* winners) {
  for (int i = 0; i < n; i++)
    if (best[i] >= 0) std::memcpy(winners + (size_t)i * 32, lists + (size_t)(off[i] + best[i]) * 32, 32);
}
}
