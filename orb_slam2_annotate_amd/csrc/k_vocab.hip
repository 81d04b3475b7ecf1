// k_vocab.hip -- the two kernels of the DBoW2 vocabulary on the device and their launchers (match_kernels.h; host side:
// vocabulary.hip): transform() (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1127-1194 feature loop, :1218-1259 k-ary descent
// with FORB::distance, FORB.cpp:81-101) and the FeatureVector of a frame.
//
// Built for the tree the reference loads -- k = 10, L = 6: 1 111 111 nodes, 53 MB of records, far beyond the L2 --
// not for a toy tree in cache (round 2 was one THREAD per descriptor chasing childOff -> childIdx -> descriptor:
// ~3 dependent scattered round trips per level and 10 separate 32-byte segments per lane and level).
//   * nodes are renumbered breadth-first: the children of a node are adjacent 48-byte records in file order, so a
//     level of the descent is ONE contiguous read (480 bytes for k = 10) with no index hop;
//   * a descriptor is descended by 16 lanes (one DPP row): lane c takes child c's record (three 16-byte requests),
//     its 256-bit Hamming distance to the query (held in 8 registers by every lane of the row), and the row takes
//     min(distance << 8 | c) by four row rotations -- the strict '<' scan of :1241-1250 keeps the FIRST minimum in
//     file order, which is the smallest key; nodes with 17..32 children take a second trip;
//   * the winner's (firstChild, nChild) -- part of the record its lane already holds -- goes to the row by
//     ds_bpermute: ONE dependent memory round trip per level, L per descriptor;
//   * each row runs U = 2 descriptors at once (independent chains, all their requests in flight together).
// Batched forms build the DBoW2::FeatureVector of every frame on the device (64-bit (node, feature) keys written by
// the transform kernel, one bitonic sort per frame in LDS).
#include <hip/hip_runtime.h>

#include "match_kernels.h"

using namespace orbfe;

namespace {

__device__ __forceinline__ uint32_t row_min_u32(uint32_t v) {  // minimum over the 16 lanes of a DPP row, in every lane
  uint32_t t;
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x128, 0xf, 0xf, false); v = t < v ? t : v;  // row_ror:8
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x124, 0xf, 0xf, false); v = t < v ? t : v;  // row_ror:4
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x122, 0xf, 0xf, false); v = t < v ? t : v;  // row_ror:2
  t = (uint32_t)__builtin_amdgcn_update_dpp((int)v, (int)v, 0x121, 0xf, 0xf, false); v = t < v ? t : v;  // row_ror:1
  return v;
}

struct NodeRec { uint4 a, b, m; };  // descriptor (a, b), m = (firstChild, nChild | positive << 8, id, word)

__device__ __forceinline__ NodeRec load_node(const VocabNode* nodes, uint32_t pos) {
  const uint4* p = reinterpret_cast<const uint4*>(nodes + pos);
  NodeRec r;
  r.a = p[0]; r.b = p[1]; r.m = p[2];
  return r;
}

__device__ __forceinline__ uint32_t hdist(const uint4 fa, const uint4 fb, const NodeRec& r) {
  return __popc(fa.x ^ r.a.x) + __popc(fa.y ^ r.a.y) + __popc(fa.z ^ r.a.z) + __popc(fa.w ^ r.a.w) +
         __popc(fb.x ^ r.b.x) + __popc(fb.y ^ r.b.y) + __popc(fb.z ^ r.b.z) + __popc(fb.w ^ r.b.w);
}

// transform(feature, word_id, weight, nid, levelsup), :1218-1259, for descriptors [0, n[f]) of every frame f.
// Workgroup = 16 rows x U descriptors; lane c of a row owns child c (and c + 16) of the row's current nodes.
// Every lane runs every iteration (the row reductions and ds_bpermute need all source lanes): rows whose
// descriptors have reached a leaf, and slots past the frame's count, just stop issuing loads.
template <int U>
__global__ __launch_bounds__(256) void k_vocab_transform16(VocabDevice v, const uint8_t* __restrict__ desc,
                                                           const int32_t* __restrict__ nPerFrame, int nFixed, int capacity,
                                                           int frameStep, int nidLevel, uint32_t* __restrict__ word,
                                                           double* __restrict__ weight, uint32_t* __restrict__ node,
                                                           unsigned long long* __restrict__ keys) {
  const int tid = threadIdx.x, c = tid & 15, row = tid >> 4, f = blockIdx.y;
  const int fi = f * frameStep;  // input slot (descriptors, count); outputs are dense per frame
  int n = nPerFrame ? nPerFrame[fi] : nFixed;
  if (n > capacity) n = capacity;
  const int base = (blockIdx.x * 16 + row) * U;
  if (blockIdx.x * 16 * U >= n && !keys) return;  // whole workgroup past the frame's count
  const size_t fo = (size_t)f * capacity, fin = (size_t)fi * capacity;
  const int laneBase = (tid & 63) & ~15;
  uint4 fa[U], fb[U];
  uint32_t first[U], cnt[U], nid[U], leafWord[U], leafPos[U], leafPositive[U];
  bool live[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const int i = base + u;
    live[u] = i < n && v.rootChildren > 0;  // an empty vocabulary leaves (0, 0, 0), :1134
    const uint4* q = reinterpret_cast<const uint4*>(desc + (fin + (size_t)(live[u] ? i : 0)) * 32);
    fa[u] = live[u] ? q[0] : make_uint4(0, 0, 0, 0);
    fb[u] = live[u] ? q[1] : make_uint4(0, 0, 0, 0);
    first[u] = 1; cnt[u] = live[u] ? v.rootChildren : 0;
    nid[u] = 0; leafWord[u] = 0; leafPos[u] = 0; leafPositive[u] = 0;
  }
  for (int level = 1;; level++) {
    bool any = false;
#pragma unroll
    for (int u = 0; u < U; u++) any |= cnt[u] > 0;
    if (!__any(any)) break;
    NodeRec r0[U] = {}, r1[U] = {};
    bool two = false;
#pragma unroll
    for (int u = 0; u < U; u++) {
      two |= cnt[u] > 16;
      if ((uint32_t)c < cnt[u]) r0[u] = load_node(v.nodes, first[u] + c);
    }
    two = __any(two);  // wave-uniform: a node with more than 16 children anywhere in the wave
    if (two) {
#pragma unroll
      for (int u = 0; u < U; u++)
        if ((uint32_t)c + 16 < cnt[u]) r1[u] = load_node(v.nodes, first[u] + c + 16);
    }
#pragma unroll
    for (int u = 0; u < U; u++) {
      uint32_t key = 0x7fffffffu;
      if ((uint32_t)c < cnt[u]) key = (hdist(fa[u], fb[u], r0[u]) << 8) | (uint32_t)c;
      if (two && (uint32_t)c + 16 < cnt[u]) {
        const uint32_t k1 = (hdist(fa[u], fb[u], r1[u]) << 8) | (uint32_t)(c + 16);
        key = k1 < key ? k1 : key;
      }
      key = row_min_u32(key);
      const uint32_t cw = key & 0xff;            // winning child, the same in every lane of the row
      const bool hi = cw >= 16;
      const int src = (laneBase + (int)(cw & 15)) << 2;
      const uint4 m = (two && hi) ? r1[u].m : r0[u].m;
      const bool act = cnt[u] > 0;               // uniform in the row
      const uint32_t pos = first[u] + cw;
      const uint32_t nf = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)m.x);
      const uint32_t nc = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)m.y);
      if (level == nidLevel) {                   // uniform in the wave
        const uint32_t id = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)m.z);
        if (act) nid[u] = id;
      }
      if (act && (nc & 0xff) == 0) {             // reached a leaf: isLeaf() ends the loop (:1257)
        leafWord[u] = (uint32_t)__builtin_amdgcn_ds_bpermute(src, (int)m.w);
        leafPos[u] = pos;
        leafPositive[u] = (nc >> 8) & 1;
      }
      if (act) { first[u] = nf; cnt[u] = nc & 0xff; }
    }
  }
  if (c == 0) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const int i = base + u;
      if (i >= capacity) continue;
      if (keys) keys[fo + i] = (live[u] && leafPositive[u]) ? (((unsigned long long)nid[u] << 32) | (unsigned)i) : ~0ull;  // "not stopped" (:1161)
      if (i >= n) continue;
      if (node) node[fo + i] = nid[u];
      if (word) {
        const int w = (int)leafWord[u];
        word[fo + i] = live[u] && w >= 0 ? (uint32_t)w : 0u;
        weight[fo + i] = live[u] ? v.weight[leafPos[u]] : 0.0;
      }
    }
  }
}

// Per frame: build the DBoW2::FeatureVector as CSR (node ids ascending; inside a node the feature indices
// ascending = addFeature order, FeatureVector.cpp:31-45) with one bitonic sort in LDS of the 64-bit keys
// (node << 32 | feature) the transform kernel wrote.
__global__ __launch_bounds__(256) void k_vocab_featvec(FeatVecBatch b) {
  extern __shared__ unsigned long long keys[];  // b.sortN entries
  __shared__ int waveTot[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, f = blockIdx.x;
  const unsigned long long* src = b.keys + (size_t)f * b.capacity;
  for (int i = tid; i < b.sortN; i += 256) keys[i] = i < b.capacity ? src[i] : ~0ull;  // padding sorts last
  __syncthreads();
  for (int k2 = 2; k2 <= b.sortN; k2 <<= 1)
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < b.sortN; i += 256) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const unsigned long long a0 = keys[i], a1 = keys[ixj];
          const bool up = (i & k2) == 0;
          if ((a0 > a1) == up) { keys[i] = a1; keys[ixj] = a0; }
        }
      }
      __syncthreads();
    }
  // segment heads -> node list + offsets; indices in sorted order
  uint32_t* nodes = b.fvNodes + (size_t)f * b.capacity;
  int32_t* offs = b.fvOffsets + (size_t)f * (b.capacity + 1);
  uint32_t* idx = b.fvIndices + (size_t)f * b.capacity;
  int run = 0, used = 0;
  for (int base = 0; base < b.sortN; base += 256) {
    const int i = base + tid;
    const unsigned long long key = i < b.sortN ? keys[i] : ~0ull;
    const bool valid = key != ~0ull;
    const bool head = valid && (i == 0 || (keys[i - 1] >> 32) != (key >> 32));
    const unsigned long long bal = __ballot(head);
    const unsigned long long balV = __ballot(valid);
    if (lane == 0) waveTot[wave] = __popcll(bal);
    __syncthreads();
    int o = run + __popcll(bal & ((1ull << lane) - 1ull));
    for (int w = 0; w < wave; w++) o += waveTot[w];
    run += waveTot[0] + waveTot[1] + waveTot[2] + waveTot[3];
    if (valid) idx[i] = (uint32_t)(key & 0xffffffffu);
    if (head) { nodes[o] = (uint32_t)(key >> 32); offs[o] = i; }
    used += __popcll(balV);  // per-wave; summed below
    __syncthreads();
  }
  // number of used features = first padding position = total valid (identical for every wave after reduction)
  __shared__ int usedTot[4];
  if (lane == 0) usedTot[wave] = used;
  __syncthreads();
  if (tid == 0) {
    const int total = usedTot[0] + usedTot[1] + usedTot[2] + usedTot[3];
    offs[run] = total;
    b.fvCount[f] = run;
  }
}

}  // namespace

namespace orbfe {
constexpr int kVocabU = 2;  // descriptors per 16-lane row
void launch_vocab_transform(hipStream_t s, const VocabDevice& v, const uint8_t* desc, const int32_t* nPerFrame, int nFixed,
                            int capacity, int frameStep, int nFrames, int nidLevel, uint32_t* word, double* weight, uint32_t* node,
                            unsigned long long* keys) {
  if (nFrames <= 0 || capacity <= 0) return;
  const int per = 16 * kVocabU, span = (nPerFrame || keys) ? capacity : nFixed;
  if (span <= 0) return;
  hipLaunchKernelGGL(k_vocab_transform16<kVocabU>, dim3((span + per - 1) / per, nFrames), dim3(256), 0, s, v, desc, nPerFrame,
                     nFixed, capacity, frameStep > 1 ? frameStep : 1, nidLevel, word, weight, node, keys);
}
void launch_vocab_featvec(hipStream_t s, const VocabDevice& v, const FeatVecBatch& b, int nFrames, int nidLevel) {
  if (nFrames <= 0) return;
  if ((size_t)b.sortN * 8 > 64 * 1024) {  // (capacity > 4096: more LDS than a launch may ask for by default; a failure
    static thread_local bool configured = false;  // is the caller's hipGetLastError())
    if (!configured)
      configured = hipFuncSetAttribute(reinterpret_cast<const void*>(k_vocab_featvec), hipFuncAttributeMaxDynamicSharedMemorySize,
                                       96 * 1024) == hipSuccess;
  }
  launch_vocab_transform(s, v, b.desc, b.n, 0, b.capacity, b.frameStep, nFrames, nidLevel, b.word, b.weight, nullptr, b.keys);
  hipLaunchKernelGGL(k_vocab_featvec, dim3(nFrames), dim3(256), (size_t)b.sortN * 8, s, b);
}
}  // namespace orbfe
