// extractor_handle.hip -- the extractor handle: its stream pool, geometry tables, HBM workspace, output block and stage
// timers, create / destroy, the getters and setters of include/orbfe.h and the back doors of host_internal.h.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/orbfe.h"
#include "extractor_handle.h"
#include "host_internal.h"
#include "kernels.h"
#include "orb_params.h"
#include "orb_pattern.inc"

using namespace orbfe;

// HIP streams of destroyed handles are kept and handed to the next handle that asks for the same role (sub-batch i, the
// two copy streams).  Two reasons.  (1) hipStreamCreate / Destroy are not free, and a process that makes one handle per
// workload or per camera re-creates the same streams again and again.  (2) Round 4 measured that the ORDER in which a process
// creates its streams matters: a HIP stream is bound to one of the GPU_MAX_HW_QUEUES hardware queues when it is created, and
// a library that creates streams of its own in between -- RCCL, when torch.distributed is initialised -- shifts that
// binding for every stream created after it: the 8-stream KITTI pipeline ran 11 % slower with the communicator created
// first (104.0 k -> 92.5 k stereo frames/s; bench.py LazyDist, tools/dist_ab.sh).  A recycled stream keeps its queue.
namespace {
struct StreamPool {
  std::mutex m;
  struct Item { int device, role; hipStream_t s; };
  std::vector<Item> items;
};
StreamPool g_streamPool;
}  // namespace
hipError_t orbfe::stream_get(int device, int role, hipStream_t* s) {
  {
    std::lock_guard<std::mutex> lk(g_streamPool.m);
    auto& v = g_streamPool.items;
    for (size_t i = 0; i < v.size(); i++)
      if (v[i].device == device && v[i].role == role) { *s = v[i].s; v.erase(v.begin() + (long)i); return hipSuccess; }
  }
  // $ORBFE_STREAM_PRIORITY = high | low: the handle's streams in a priority class of their own (its own set of hardware
  // queues in the HIP runtime), so that streams other libraries create at normal priority cannot shift their binding
  static const int kPrioEnv = [] {
    const char* v = getenv("ORBFE_STREAM_PRIORITY");
    return !v ? 0 : (std::string(v) == "high" ? 1 : (std::string(v) == "low" ? 2 : 0));
  }();
  if (kPrioEnv) {
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess && least != greatest)
      return hipStreamCreateWithPriority(s, hipStreamNonBlocking, kPrioEnv == 1 ? greatest : least);
    (void)hipGetLastError();
  }
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

namespace {

void stream_put(int device, int role, hipStream_t s) {
  if (!s) return;
  (void)hipStreamSynchronize(s);
  {
    std::lock_guard<std::mutex> lk(g_streamPool.m);
    if (g_streamPool.items.size() < 256) { g_streamPool.items.push_back({device, role, s}); return; }
  }
  (void)hipStreamDestroy(s);
}

// Streams and events of sub-batches [e->subsReady, n) are created on first use: a handle for one live camera (1 stream)
// costs 1 stream + 136 events to create instead of 32 streams + ~4 300 events.
int ensure_subs(orbfe_extractor* e, int n) {
  if (n > orbfe_extractor::kMaxStreams) n = orbfe_extractor::kMaxStreams;
  // $ORBFE_STREAM_SKEW = k (experiment, tools/skew_ab.sh): k idle streams are created in front of the handle's first extra
  // stream, shifting the hardware-queue binding of everything created after them -- what a library like RCCL does by accident
  static const int kSkew = getenv("ORBFE_STREAM_SKEW") ? atoi(getenv("ORBFE_STREAM_SKEW")) : 0;
  static bool skewed = false;
  if (kSkew > 0 && !skewed && n > 1) {
    skewed = true;
    for (int k = 0; k < kSkew; k++) { hipStream_t dummy; (void)hipStreamCreateWithFlags(&dummy, hipStreamNonBlocking); }
  }
  for (int i = e->subsReady; i < n; i++) {
    if (i > 0 && !e->extra[i - 1]) HIPCHK(stream_get(e->device, i, &e->extra[i - 1]));
    HIPCHK(hipEventCreateWithFlags(&e->evStat[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->evChunkDone[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->evPyr[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->evFast[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->evBlur[i], hipEventDisableTiming));
    HIPCHK(hipEventCreateWithFlags(&e->evTail[i], hipEventDisableTiming));
    for (int r = 0; r < orbfe_extractor::kEvRing; r++)
      for (int st = 0; st < ORBFE_STAGE_COUNT; st++) {
        HIPCHK(hipEventCreate(&e->evA[r][i][st]));
        HIPCHK(hipEventCreate(&e->evB[r][i][st]));
      }
    e->subsReady = i + 1;
  }
  return ORBFE_OK;
}

void free_geometry(orbfe_extractor* e) {
  e->d_cells.reset();
  e->d_lvgeom.reset();
  e->d_descTiles.reset();
  e->nDescTiles = 0;
  e->d_chainTiles.reset();
  e->nChainTiles = 0;
  e->chainOk = false;
  for (int l = 0; l < kMaxLevels; l++) {
    e->d_xofs[l].reset(); e->d_alpha[l].reset(); e->d_yofs[l].reset(); e->d_beta[l].reset();
    e->d_colrec[l].reset(); e->d_rowrec[l].reset(); e->d_tileGx[l].reset(); e->d_tileDy[l].reset();
  }
}
void free_workspace(orbfe_extractor* e) {
  e->d_pyr.reset(); e->d_blur.reset(); e->d_slots.reset(); e->d_cand.reset();
  e->d_cellCount.reset(); e->d_cellPrefix.reset(); e->d_candCount.reset(); e->d_nodeOf.reset();
  e->d_levelKp.reset(); e->d_levelCount.reset(); e->d_octreeWork.reset();
  e->octreeWorkStride = 0;
  e->capFrames = 0;
}
// host wait for the last frame build that reads the output block (before the block is freed, or as part of sync_all)
int reader_settle(orbfe_extractor* e) {
  if (!e->readerPending) return ORBFE_OK;
  HIPCHK(hipEventSynchronize(e->evReaderDone));
  e->readerPending = false;
  return ORBFE_OK;
}
void free_outputs(orbfe_extractor* e) {
  (void)reader_settle(e);
  e->d_outBlock.reset();
  e->d_kpOut = nullptr; e->d_descOut = nullptr; e->d_nOut = nullptr;
  e->outCap = 0;
  e->outLastFrames = 0;
}

// k_pyramid_chain: 32 x 32 tiles of levels 1 .. n-1, each with the rectangles it needs of the levels below it
// (walking the cv::resize tables back to level 0); usable (ok) while the two LDS rectangle buffers fit
struct ChainPlan {
  std::vector<ChainTile> tiles;
  size_t bufA = 0, bufB = 0;
  int maxW = 0, maxH = 0;
  bool ok = false;
};
ChainPlan build_chain_tiles(const FrameGeom& g) {
  ChainPlan c;
  bool ok = g.nlevels > 1;
  for (int l = g.nlevels - 1; l >= 1 && ok; l--) {  // the longest chains first
    const int TS = l >= 4 ? 16 : 32;  // (deep levels: smaller tiles, i.e. smaller rectangles to recompute -- 16 measured best of 32 / 16 / 8)
    for (int y0 = 0; y0 < g.lv[l].h && ok; y0 += TS)
      for (int x0 = 0; x0 < g.lv[l].w; x0 += TS) {
        ChainTile t = {};
        t.level = l;
        int rx0 = x0, ry0 = y0, rx1 = std::min(x0 + TS, g.lv[l].w) - 1, ry1 = std::min(y0 + TS, g.lv[l].h) - 1;  // inclusive
        for (int k = l; k >= 0; k--) {
          const int w = rx1 - rx0 + 1, h = ry1 - ry0 + 1;
          if (w > 255 || h > 255) { ok = false; break; }
          t.r[k] = ChainRect{(int16_t)rx0, (int16_t)ry0, (int16_t)w, (int16_t)h};
          const size_t bytes = (size_t)((w + 3) & ~3) * h;
          if (k & 1) c.bufB = std::max(c.bufB, bytes); else c.bufA = std::max(c.bufA, bytes);
          if (k > 0) { c.maxW = std::max(c.maxW, w); c.maxH = std::max(c.maxH, h); }  // (table entries of the level-k output rectangle)
          if (k == 0) break;
          const ResizeTables& z = g.rz[k];
          const int Wp = g.lv[k - 1].w, Hp = g.lv[k - 1].h;
          auto clampr = [&](int v) { return v < 0 ? 0 : (v >= Hp ? Hp - 1 : v); };
          const int sx0 = z.xofs[rx0], sx1 = std::min(z.xofs[rx1] + 1, Wp - 1);
          const int sy0 = clampr(z.yofs[ry0]), sy1 = clampr(z.yofs[ry1] + 1);
          rx0 = sx0; rx1 = std::max(sx1, sx0); ry0 = sy0; ry1 = std::max(sy1, sy0);
        }
        if (!ok) break;
        c.tiles.push_back(t);
      }
  }
  c.bufA = (c.bufA + 15) & ~(size_t)15;
  c.bufB = (c.bufB + 15) & ~(size_t)15;
  if (ok && c.bufA + c.bufB + (size_t)(c.maxW + c.maxH) * 8 > (size_t)60 * 1024) ok = false;
  c.ok = ok && !c.tiles.empty();
  return c;
}

}  // namespace

int orbfe::ensure_geometry(orbfe_extractor* e, int W, int H) {
  if (e->geom.W == W && e->geom.H == H && e->d_lvgeom) return ORBFE_OK;
  if (W > 32767 || H > 32767)  // signed 16-bit node rectangles in k_octree (unsigned 16-bit coordinates elsewhere)
    return fail(ORBFE_ERR_INVALID, "images larger than 32767 x 32767 are not supported");
  free_geometry(e);
  free_workspace(e);
  e->haveLast = false;
  e->geom.build(e->tab, W, H);
  const FrameGeom& g = e->geom;
  for (const CellDesc& c : g.cells)
    if (c.w > 60 || c.h > 60) return fail(ORBFE_ERR_INVALID, "FAST grid cell larger than 60 px");
  for (int l = 0; l < g.nlevels; l++)
    if (g.lv[l].w < 1 || g.lv[l].h < 1) return fail(ORBFE_ERR_INVALID, "image too small for the pyramid");
  const int maxL = octree_node_capacity(g.lv, g.nlevels);
  if (maxL == 0) return fail(ORBFE_ERR_INVALID, "level too large for the octree kernel");
  if (maxL < 0) return fail(ORBFE_ERR_INVALID, "nfeatures too large: more than 65532 keypoints on one pyramid level");
  e->octreeMaxL = maxL;  // octree_lds_bytes(maxL) > kOctreeLdsLimit: node lists in global memory (ensure_workspace)
  int rc;
  if ((rc = e->d_cells.upload(g.cells))) return rc;
  if ((rc = e->d_lvgeom.upload(g.lv, (size_t)kMaxLevels))) return rc;
  const std::vector<DescTile> descTiles = build_desc_tiles(g.lv, g.nlevels);
  e->nDescTiles = (int)descTiles.size();
  if (!descTiles.empty() && (rc = e->d_descTiles.upload(descTiles))) return rc;
  const ChainPlan chain = build_chain_tiles(g);
  if (chain.ok) {
    if ((rc = e->d_chainTiles.upload(chain.tiles))) return rc;
    e->nChainTiles = (int)chain.tiles.size();
    e->chainBufA = (int)chain.bufA; e->chainBufB = (int)chain.bufB; e->chainMaxW = chain.maxW; e->chainMaxH = chain.maxH;
    e->chainOk = true;
  }
  for (int l = 1; l < g.nlevels; l++) {
    const ResizeTables& t = g.rz[l];
    if ((rc = e->d_xofs[l].upload(t.xofs)) || (rc = e->d_alpha[l].upload(t.alpha))) return rc;
    if ((rc = e->d_yofs[l].upload(t.yofs)) || (rc = e->d_beta[l].upload(t.beta))) return rc;
    if (t.colrec.empty()) continue;
    if ((rc = e->d_colrec[l].upload(t.colrec)) || (rc = e->d_rowrec[l].upload(t.rowrec))) return rc;
    if (t.tileGx.empty()) continue;
    if ((rc = e->d_tileGx[l].upload(t.tileGx)) || (rc = e->d_tileDy[l].upload(t.tileDy))) return rc;
  }
  return ORBFE_OK;
}

int orbfe::ensure_workspace(orbfe_extractor* e, int nFrames) {
  if (nFrames <= e->capFrames) return ORBFE_OK;
  free_workspace(e);
  const FrameGeom& g = e->geom;
  const size_t B = (size_t)nFrames;
  int rc;
  if ((rc = e->d_pyr.alloc(B * g.pyrBytes))) return rc;
  if ((rc = e->d_blur.alloc(B * g.pyrBytes))) return rc;
  if ((rc = e->d_slots.alloc(B * (size_t)g.totalSlots))) return rc;
  if ((rc = e->d_cand.alloc(B * (size_t)g.totalSlots))) return rc;
  if ((rc = e->d_cellCount.alloc(B * g.cells.size()))) return rc;
  if ((rc = e->d_cellPrefix.alloc(B * g.cells.size()))) return rc;
  if ((rc = e->d_candCount.alloc(B * (size_t)g.nlevels))) return rc;
  if ((rc = e->d_nodeOf.alloc(B * (size_t)g.totalSlots))) return rc;
  if ((rc = e->d_levelKp.alloc(B * (size_t)g.totalKpCap))) return rc;
  if ((rc = e->d_levelCount.alloc(B * (size_t)g.nlevels))) return rc;
  if (octree_lds_bytes(e->octreeMaxL) > kOctreeLdsLimit) {
    e->octreeWorkStride = octree_work_stride(e->octreeMaxL);
    if ((rc = e->d_octreeWork.alloc(B * (size_t)g.nlevels * e->octreeWorkStride))) return rc;
  }
  e->capFrames = nFrames;
  return ORBFE_OK;
}

int orbfe::ensure_outputs(orbfe_extractor* e, int nFrames, int capacity) {
  const int need = nFrames * capacity;
  if (need == e->outCap && e->d_nOut) return ORBFE_OK;  // exact layout: a small batch stays one compact block
  free_outputs(e);
  int rc;
  const size_t kpBytes = ((size_t)need * sizeof(orbfe_keypoint) + 255) & ~(size_t)255;
  const size_t descBytes = ((size_t)need * 32 + 255) & ~(size_t)255;
  const size_t cntBytes = (size_t)(nFrames > 4096 ? nFrames : 4096) * 4;
  if ((rc = e->d_outBlock.alloc(kpBytes + descBytes + cntBytes))) return rc;
  e->d_kpOut = reinterpret_cast<orbfe_keypoint*>(e->d_outBlock.p);
  e->d_descOut = e->d_outBlock + kpBytes;
  e->d_nOut = reinterpret_cast<int32_t*>(e->d_outBlock + kpBytes + descBytes);
  e->outCap = need;
  return ORBFE_OK;
}

static void resolve_slot(orbfe_extractor* e, int slot) {
  for (int sub = 0; sub < orbfe_extractor::kEvSubs; sub++)
    for (int st = 0; st < ORBFE_STAGE_COUNT; st++) {
      StageInterval& iv = e->ev[slot][sub][st];
      if (!iv.used) continue;
      iv.used = false;
      float ms = 0;
      if (hipEventSynchronize(e->evB[slot][sub][st]) == hipSuccess &&
          hipEventElapsedTime(&ms, e->evA[slot][sub][st], e->evB[slot][sub][st]) == hipSuccess) {
        e->stageMs[st] += ms;
        e->stageLaunches[st] += iv.launches;
        e->stageFrames[st] += iv.frames;
      }
    }
}
void orbfe::resolve_stage_times(orbfe_extractor* e) {
  for (int slot = 0; slot < orbfe_extractor::kEvRing; slot++) resolve_slot(e, slot);
}
// advance to the next ring slot before a call records into it (waits for the call kEvRing calls back that used it)
void orbfe::next_event_slot(orbfe_extractor* e) {
  if (!e->stageMask) return;
  e->evSlot = (e->evSlot + 1) % orbfe_extractor::kEvRing;
  resolve_slot(e, e->evSlot);
}

// host wait for everything the handle has enqueued, and for the frame build that reads its output block
int orbfe::sync_all(orbfe_extractor* e) {
  HIPCHK(hipStreamSynchronize(e->stream));
  for (int i = 0; i < orbfe_extractor::kMaxStreams - 1; i++)
    if (e->extra[i]) HIPCHK(hipStreamSynchronize(e->extra[i]));
  return reader_settle(e);
}

extern "C" int orbfe_extractor_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                                      int minThFAST, int device, orbfe_extractor** out) {
  if (!out) return fail(ORBFE_ERR_INVALID, "out is NULL");
  *out = nullptr;
  if (nfeatures < 0 || nlevels < 1 || nlevels > ORBFE_MAX_LEVELS || !(scaleFactor > 1.0f))
    return fail(ORBFE_ERR_INVALID, "bad extractor parameters");
  int ndev = 0;
  HIPCHK(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev) return fail(ORBFE_ERR_HIP, "no such HIP device");
  HIPCHK(hipSetDevice(device));
  orbfe_extractor* e = new (std::nothrow) orbfe_extractor();
  if (!e) return fail(ORBFE_ERR_NOMEM, "out of memory");
  e->device = device;
  e->tab.init(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
  // defaults from the environment (the setters override them)
  if (const char* env = getenv("ORBFE_COPY_UNALIGNED")) e->copyUnaligned = atoi(env) != 0;
  if (const char* env = getenv("ORBFE_FAST_MODE")) {
    const std::string v(env);
    e->fastMode = v == "high" ? 1 : (v == "low" ? 2 : 0);
  }
  if (const char* env = getenv("ORBFE_LANES")) e->laneMode = atoi(env) != 0;
  if (const char* env = getenv("ORBFE_FUSED")) e->fused = atoi(env) != 0;
  if (const char* env = getenv("ORBFE_PYRBLUR")) e->pyrBlur = atoi(env) != 0;
  if (const char* env = getenv("ORBFE_PYR_CHAIN")) e->pyrChain = atoi(env) != 0;
  if (const char* env = getenv("ORBFE_BLUR_SPEC")) {
    const int v = atoi(env);
    if (v >= 0 && v <= 2) e->blurSpec = v;
  }
  if (const char* env = getenv("ORBFE_STREAMS")) {
    int v = atoi(env);
    if (v >= 1 && v <= orbfe_extractor::kMaxStreams) e->nStreams = v;
  }
  float4 patF[256];
  // test i = (x0, y0, x1, y1) in the table; uploaded as (x0, x1, y0, y1) so that k_orient_desc rotates the
  // two points of a test in one packed-fp32 operation per product
  for (int i = 0; i < 256; i++)
    patF[i] = make_float4((float)kOrbBitPattern31[4 * i + 0], (float)kOrbBitPattern31[4 * i + 2],
                          (float)kOrbBitPattern31[4 * i + 1], (float)kOrbBitPattern31[4 * i + 3]);
  uint4 momTab[64];
  build_moment_table(reinterpret_cast<uint8_t*>(momTab));
  float scTab[2 * kMaxLevels] = {};
  for (int i = 0; i < e->tab.nlevels; i++) { scTab[i] = e->tab.scale[i]; scTab[kMaxLevels + i] = e->tab.invScale[i]; }
  const size_t nStat = (size_t)orbfe_extractor::kMaxStreams * orbfe_extractor::kStatSlots;
  auto init = [&]() -> int {
    int rc;
    HIPCHK(stream_get(device, 0, &e->stream));
    if ((rc = e->d_fastStat.alloc(nStat)) || (rc = e->h_fastStat.alloc(nStat))) return rc;
    HIPCHK(hipEventCreateWithFlags(&e->evConsumerDone, hipEventDisableTiming));
    if ((rc = ensure_subs(e, e->nStreams > 3 ? e->nStreams : 3))) return rc;  // 3: the lane schedule's P / V / T
    if ((rc = e->d_patternF.upload(patF, 256)) || (rc = e->d_scaleTab.upload(scTab, 2 * kMaxLevels))) return rc;
    if ((rc = e->d_momentTab.upload(momTab, 64))) return rc;
    return e->d_umax.upload(e->tab.umax, 16);
  };
  if (int rc = init()) {
    const std::string why = orbfe_last_error();
    orbfe_extractor_destroy(e);
    return fail(rc, "extractor_create: " + why);
  }
  *out = e;
  return ORBFE_OK;
}

extern "C" void orbfe_extractor_destroy(orbfe_extractor* e) {
  if (!e) return;
  (void)hipSetDevice(e->device);
  if (e->stream) (void)hipStreamSynchronize(e->stream);
  for (int i = 0; i < orbfe_extractor::kMaxStreams - 1; i++)
    if (e->extra[i]) stream_put(e->device, i + 1, e->extra[i]);
  stream_put(e->device, kRoleH2D, e->sH2D);
  stream_put(e->device, kRoleD2H, e->sD2H);
  free_geometry(e);
  free_workspace(e);
  free_outputs(e);  // (settles the reader first; every other buffer goes with the handle below)
  auto drop = [](hipEvent_t ev) { if (ev) (void)hipEventDestroy(ev); };
  for (int i = 0; i < orbfe_extractor::kMaxStreams; i++) {
    drop(e->evStat[i]); drop(e->evChunkDone[i]); drop(e->evPyr[i]); drop(e->evFast[i]); drop(e->evBlur[i]); drop(e->evTail[i]);
  }
  for (int i = 0; i < 2; i++) { drop(e->evIn[i]); drop(e->evComp[i]); drop(e->evOutDone[i]); }
  for (int r = 0; r < orbfe_extractor::kEvRing; r++)
    for (int u = 0; u < orbfe_extractor::kEvSubs; u++)
      for (int i = 0; i < ORBFE_STAGE_COUNT; i++) { drop(e->evA[r][u][i]); drop(e->evB[r][u][i]); }
  drop(e->evConsumerDone);
  drop(e->evReaderDone);
  stream_put(e->device, 0, e->stream);
  delete e;
}

extern "C" int orbfe_extractor_synchronize(orbfe_extractor* e) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  HIPCHK(hipSetDevice(e->device));
  int rc = sync_all(e);
  if (rc) return rc;
  resolve_stage_times(e);
  return ORBFE_OK;
}

extern "C" int orbfe_extractor_get_levels(const orbfe_extractor* e) { return e ? e->tab.nlevels : 0; }
extern "C" float orbfe_extractor_get_scale_factor(const orbfe_extractor* e) { return e ? (float)e->tab.scaleFactor : 0.f; }
#define GETTER(name, field)                                                       \
  extern "C" int name(const orbfe_extractor* e, float* out) {                     \
    if (!e || !out) return fail(ORBFE_ERR_INVALID, #name ": NULL argument");      \
    for (int i = 0; i < e->tab.nlevels; i++) out[i] = e->tab.field[i];            \
    return ORBFE_OK;                                                              \
  }
GETTER(orbfe_extractor_get_scale_factors, scale)
GETTER(orbfe_extractor_get_inverse_scale_factors, invScale)
GETTER(orbfe_extractor_get_scale_sigma_squares, sigma2)
GETTER(orbfe_extractor_get_inverse_scale_sigma_squares, invSigma2)
extern "C" int orbfe_extractor_get_features_per_level(const orbfe_extractor* e, int32_t* out) {
  if (!e || !out) return fail(ORBFE_ERR_INVALID, "NULL argument");
  for (int i = 0; i < e->tab.nlevels; i++) out[i] = e->tab.quota[i];
  return ORBFE_OK;
}
extern "C" int orbfe_extractor_get_umax(const orbfe_extractor* e, int32_t* out16) {
  if (!e || !out16) return fail(ORBFE_ERR_INVALID, "NULL argument");
  for (int i = 0; i < 16; i++) out16[i] = e->tab.umax[i];
  return ORBFE_OK;
}
extern "C" int orbfe_extractor_max_keypoints(const orbfe_extractor* e) {
  if (!e) return 0;
  // quota + 3 per level, or 4 root children per level on very wide images (nIni <= 16 assumed)
  int n = 0;
  for (int l = 0; l < e->tab.nlevels; l++) n += (e->tab.quota[l] + 3 > 64 ? e->tab.quota[l] + 3 : 64);
  return n;
}
extern "C" int orbfe_extractor_max_keypoints_for(const orbfe_extractor* e, int width, int height) {
  if (!e || width <= 0 || height <= 0) return 0;
  if (e->geom.W == width && e->geom.H == height && e->geom.totalKpCap > 0) return e->geom.totalKpCap;  // current geometry
  FrameGeom g;  // the exact bound of the pipeline for this image size: per level max(quota + 3, 4 * nIni)
  g.build(e->tab, width, height);
  return g.totalKpCap;
}
extern "C" int orbfe_extractor_level_size(const orbfe_extractor* e, int width, int height, int level, int* w, int* h) {
  if (!e || !w || !h || level < 0 || level >= e->tab.nlevels) return fail(ORBFE_ERR_INVALID, "bad argument");
  const float s = e->tab.invScale[level];
  *w = cv_round((float)width * s);
  *h = cv_round((float)height * s);
  return ORBFE_OK;
}

// internal (frames.hip, orbfe_frame_from_extractor): device records of frame `frame` of the last host-buffer call
extern "C" int orbfe_extractor_output_device_(orbfe_extractor* e, int frame, const orbfe_keypoint** d_kp, const uint8_t** d_desc,
                                              int* n, int* device) {
  if (!e || !d_kp || !d_desc || !n || !device) return fail(ORBFE_ERR_INVALID, "frame_from_extractor: NULL argument");
  if (e->outLastFrames <= 0)
    return fail(ORBFE_ERR_INVALID, "frame_from_extractor: the handle holds no output block (the last call was not orbfe_extract / a small "
                                   "orbfe_extract_batch; device-batch callers own their outputs: orbfe_frame_from_device)");
  if (frame < 0 || frame >= e->outLastFrames) return fail(ORBFE_ERR_INVALID, "frame_from_extractor: frame out of range");
  *d_kp = e->d_kpOut + (size_t)frame * e->outLastCapacity;
  *d_desc = e->d_descOut + (size_t)frame * e->outLastCapacity * 32;
  *n = e->outLastCount[(size_t)frame];
  *device = e->device;
  return ORBFE_OK;
}

extern "C" int orbfe_extractor_profile(orbfe_extractor* e, int stage_mask) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  HIPCHK(hipSetDevice(e->device));
  { int rcs = sync_all(e); if (rcs) return rcs; }
  resolve_stage_times(e);
  e->stageMask = stage_mask < 0 ? 0xffffffffu : (unsigned)stage_mask;
  for (int i = 0; i < ORBFE_STAGE_COUNT; i++) { e->stageMs[i] = 0; e->stageLaunches[i] = 0; e->stageFrames[i] = 0; }
  return ORBFE_OK;
}
extern "C" int orbfe_extractor_profile_get(orbfe_extractor* e, double* ms_out, int64_t* launches_out,
                                           double* frames_out) {
  if (!e || !ms_out || !launches_out) return fail(ORBFE_ERR_INVALID, "NULL argument");
  for (int i = 0; i < ORBFE_STAGE_COUNT; i++) {
    ms_out[i] = e->stageMs[i];
    launches_out[i] = e->stageLaunches[i];
    if (frames_out) frames_out[i] = e->stageFrames[i];
  }
  return ORBFE_OK;
}
extern "C" const char* orbfe_stage_name(int stage) {
  static const char* names[ORBFE_STAGE_COUNT] = {"h2d", "pyramid", "fast", "octree", "blur", "orient_desc", "d2h", "match"};
  return (stage >= 0 && stage < ORBFE_STAGE_COUNT) ? names[stage] : "?";
}

// internal (vocabulary.hip): a consumer of the last extract call's outputs that runs on the handle's own
// stream.  begin: stream 0 waits (on the device) for every sub-batch stream of that call and is returned;
// end: marks the consumer's last kernel so that the next extract call's sub-batch streams wait for it.
extern "C" int orbfe_extractor_consumer_begin_(orbfe_extractor* e, hipStream_t* s) {
  if (!e || !s) return fail(ORBFE_ERR_INVALID, "NULL handle");
  HIPCHK(hipSetDevice(e->device));
  for (int i = 1; i < e->chunksPending; i++) HIPCHK(hipStreamWaitEvent(e->stream, e->evChunkDone[i], 0));
  *s = e->stream;
  e->stage_open(ORBFE_STAGE_MATCH, 0, e->stream, 1, e->last.frames);  // same ring slot as the extract call it follows, sub-batch 0
  return ORBFE_OK;
}
extern "C" int orbfe_extractor_consumer_end_(orbfe_extractor* e) {
  e->stage_close(ORBFE_STAGE_MATCH, 0, e->stream);
  HIPCHK(hipEventRecord(e->evConsumerDone, e->stream));
  e->consumerPending = true;
  return ORBFE_OK;
}

// internal (frames.hip, orbfe_frame_from_extractor): a frame build that reads the output block was enqueued on `s`;
// the next call that writes the block waits for it on the device.  Builds on one stream are ordered by that stream, so
// one event covers them; a build on another thread's stream first settles the one before it (rare: one handle, two threads)
extern "C" int orbfe_extractor_reader_end_(orbfe_extractor* e, hipStream_t s) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  HIPCHK(hipSetDevice(e->device));
  if (!e->evReaderDone) HIPCHK(hipEventCreateWithFlags(&e->evReaderDone, hipEventDisableTiming));
  if (e->readerPending && e->readerStream != s) { int rc = reader_settle(e); if (rc) return rc; }
  HIPCHK(hipEventRecord(e->evReaderDone, s));
  e->readerStream = s;
  e->readerPending = true;
  return ORBFE_OK;
}

// internal (vocabulary.hip): how the last extract call was split, so that a batched matcher can work per sub-batch on
// the sub-batch's own stream.  streams / chunkDone: kMaxStreams entries.
extern "C" int orbfe_extractor_split_(orbfe_extractor* e, SubSplit* split, hipStream_t* streams, hipEvent_t* chunkDone) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  HIPCHK(hipSetDevice(e->device));
  *split = e->last;
  if (!e->haveLast) split->S = 0;
  for (int i = 0; i < orbfe_extractor::kMaxStreams; i++) {
    streams[i] = i == 0 ? e->stream : e->extra[i - 1];
    chunkDone[i] = e->evChunkDone[i];
  }
  return ORBFE_OK;
}
// internal: stage-timer marks for work another translation unit enqueues on a sub-batch stream
extern "C" void orbfe_extractor_stage_mark_(orbfe_extractor* e, int stage, int sub, int isEnd, hipStream_t s, int frames) {
  if (!e) return;
  if (isEnd) e->stage_close(stage, sub, s);
  else e->stage_open(stage, sub, s, 1, frames);
}

// Debug: route DistributeOctTree through the host implementation (cross-check of k_octree).
extern "C" int orbfe_extractor_debug_host_octree(orbfe_extractor* e, int enable) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  e->hostOctree = enable != 0;
  return ORBFE_OK;
}

// A setter of one field of an idle handle: `ok` checks the value, `assign` stores it once every stream is drained.
#define SETTER(name, arg, ok, why, assign)                                   \
  extern "C" int name(orbfe_extractor* e, int arg) {                         \
    if (!e || !(ok)) return fail(ORBFE_ERR_INVALID, e ? why : "NULL handle"); \
    HIPCHK(hipSetDevice(e->device));                                         \
    int rc = sync_all(e);                                                    \
    if (rc) return rc;                                                       \
    assign;                                                                  \
    return ORBFE_OK;                                                         \
  }
// FAST threshold order: 0 = auto, 1 = iniThFAST first with per-cell fallback, 2 = one attempt at the lower threshold.
SETTER(orbfe_extractor_set_fast_mode, mode, mode >= 0 && mode <= 2, "set_fast_mode: 0 (auto), 1 (high first) or 2 (low first)", {
  e->fastMode = mode;
  for (int i = 0; i < orbfe_extractor::kMaxStreams; i++) e->statPending[i] = false;
})
// Which OpenCV's GaussianBlur arithmetic the extractor reproduces (include/orbfe.h, ORBFE_BLUR_*).
SETTER(orbfe_extractor_set_blur_spec, spec, spec >= 0 && spec <= 2,
       "set_blur_spec: 0 (OpenCV >= 3.4.1/4.x), 1 (2.4/3.x scalar) or 2 (2.4/3.x SSE2)", e->blurSpec = spec)
// GaussianBlur inside the FAST kernel (1; $ORBFE_FUSED) or as the separate k_blur7 launch (0, the default).  Identical results.
SETTER(orbfe_extractor_set_fused, enable, true, "", e->fused = enable != 0)
// ComputePyramid and the per-level GaussianBlur as ONE kernel per level (1, the default; $ORBFE_PYRBLUR) or as the
// separate resize and blur launches (0).  Identical results.
SETTER(orbfe_extractor_set_pyramid_blur, enable, true, "", e->pyrBlur = enable != 0)
// The pyramid of a call of <= 8 frames in ONE launch (k_pyramid_chain) instead of n-1 dependent resize launches.  Identical
// results; off by default (measured: no faster).
SETTER(orbfe_extractor_set_pyramid_chain, enable, true, "", e->pyrChain = enable != 0)
// Schedule of the sub-batches of a call: 0 = one independent stream per sub-batch, 1 = three lanes shared by all
// sub-batches (pyramid | FAST + blur | gather + octree + orientation/descriptors) as a software pipeline.
SETTER(orbfe_extractor_set_schedule, lanes, true, "", e->laneMode = lanes != 0)
// Number of sub-batch streams one call is split over (1..32; default 1, or $ORBFE_STREAMS).
SETTER(orbfe_extractor_set_streams, n, n >= 1 && n <= orbfe_extractor::kMaxStreams, "set_streams: 1..32", {
  if ((rc = ensure_subs(e, n))) return rc;
  e->nStreams = n;
})

// Orientation + descriptor stage in tile form (1), per-keypoint form (0) or as $ORBFE_DESC_TILES says (< 0, the default);
// read per call, so no drain.
extern "C" int orbfe_extractor_set_desc_tiles(orbfe_extractor* e, int enable) {
  if (!e) return fail(ORBFE_ERR_INVALID, "NULL handle");
  e->descTilesMode = enable < 0 ? -1 : (enable ? 1 : 0);
  return ORBFE_OK;
}
