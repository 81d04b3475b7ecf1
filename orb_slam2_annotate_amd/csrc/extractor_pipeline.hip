// extractor_pipeline.hip -- the schedule of one extract call: what run_chunk enqueues for a sub-batch, how run_pipeline
// splits a call over streams or lanes and orders it against the previous call's readers, and the prologue of every call.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdlib>
#include <thread>
#include <vector>

#include "../../include/orbfe.h"
#include "extractor_handle.h"
#include "host_internal.h"
#include "kernels.h"
#include "octree_host.h"
#include "orb_params.h"

using namespace orbfe;

// Debug cross-check only: DistributeOctTree on the host (octree_host.cpp) with a D2H/H2D round trip.
static int run_host_octree(orbfe_extractor* e, int nFrames) {
  const FrameGeom& g = e->geom;
  hipStream_t s = e->stream;
  {
    const int nl = g.nlevels;
    e->h_candCount.resize((size_t)nFrames * nl);
    HIPCHK(hipMemcpyAsync(e->h_candCount.data(), e->d_candCount, sizeof(int32_t) * nFrames * nl, hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    std::vector<size_t> off((size_t)nFrames * nl + 1, 0);
    for (size_t i = 0; i < (size_t)nFrames * nl; i++) off[i + 1] = off[i] + (size_t)e->h_candCount[i];
    e->h_cand.resize(off.back() + 1);
    for (int f = 0; f < nFrames; f++)
      for (int l = 0; l < nl; l++) {
        const size_t i = (size_t)f * nl + l;
        if (e->h_candCount[i] > 0)
          HIPCHK(hipMemcpyAsync(e->h_cand.data() + off[i], e->d_cand + (size_t)f * g.totalSlots + g.lv[l].slotStart,
                                sizeof(Candidate) * e->h_candCount[i], hipMemcpyDeviceToHost, s));
      }
    HIPCHK(hipStreamSynchronize(s));
    e->h_levelKp.assign((size_t)nFrames * g.totalKpCap, LevelKp{0, 0, 0, 0});
    e->h_levelCount.assign((size_t)nFrames * nl, 0);
    std::atomic<int> next{0};
    const int nTasks = nFrames * nl;
    auto worker = [&]() {
      for (;;) {
        const int i = next.fetch_add(1);
        if (i >= nTasks) break;
        const int f = i / nl, l = i % nl;
        const LevelGeom& lg = g.lv[l];
        const int n = distribute_octree_host(e->h_cand.data() + off[i], e->h_candCount[i], kMinBorder,
                                             lg.w - kEdgeThreshold + 3, kMinBorder, lg.h - kEdgeThreshold + 3,
                                             lg.quota, e->h_levelKp.data() + (size_t)f * g.totalKpCap + lg.kpStart, lg.kpCap);
        e->h_levelCount[i] = n > lg.kpCap ? lg.kpCap : n;
      }
    };
    unsigned hw = std::thread::hardware_concurrency();
    int nThreads = (int)(hw ? hw : 4);
    if (nThreads > 16) nThreads = 16;
    if (nThreads > nTasks) nThreads = nTasks;
    std::vector<std::thread> pool;
    for (int i = 1; i < nThreads; i++) pool.emplace_back(worker);
    worker();
    for (auto& th : pool) th.join();
    HIPCHK(hipMemcpyAsync(e->d_levelKp, e->h_levelKp.data(), sizeof(LevelKp) * e->h_levelKp.size(), hipMemcpyHostToDevice, s));
    HIPCHK(hipMemcpyAsync(e->d_levelCount, e->h_levelCount.data(), sizeof(int32_t) * e->h_levelCount.size(), hipMemcpyHostToDevice, s));
  }
  return ORBFE_OK;
}

// The device pipeline for frames [f0, f0+nFrames) of a call, enqueued on stream `s`.
// $ORBFE_KNOCKOUT = bit mask of stages whose launches are SKIPPED once the handle has run $ORBFE_KNOCKOUT_AFTER (default 4)
// chunks in full (1 pyramid + blur, 2 FAST, 4 gather + octree, 8 orientation + descriptors, 16 stereo matcher): a timing
// experiment -- how much does a stage add to the PIPELINED step? (tools/knockout.sh; the skipped stage's outputs are
// the previous step's, so everything downstream still runs on real data; results unchecked, ORBFE_BENCH_NO_CHECK)
int orbfe::knockout_mask(orbfe_extractor* e, bool count) {
  static const int kMask = getenv("ORBFE_KNOCKOUT") ? atoi(getenv("ORBFE_KNOCKOUT")) : 0;
  static const int kAfter = getenv("ORBFE_KNOCKOUT_AFTER") ? atoi(getenv("ORBFE_KNOCKOUT_AFTER")) : 4;
  if (!kMask) return 0;
  if (count) e->knockoutChunks++;
  return e->knockoutChunks > kAfter ? kMask : 0;
}

// level0: view of the call's input frames in HBM (frame 0 of the call).
static int run_chunk(orbfe_extractor* e, hipStream_t s, int sub, LevelView level0, int f0, int nFrames,
                     orbfe_keypoint* d_kp, uint8_t* d_desc, int capacity, int32_t* d_nOut, PyramidViews* pyrOut,
                     PyramidViews* blurOut, hipStream_t sV = nullptr, hipStream_t sT = nullptr) {
  // lanes: pyramid on s (= P), FAST + blur on sV, gather / octree / orientation + descriptors on sT; one stream
  // for everything when sV is NULL
  const bool lanes = sV != nullptr;
  if (!lanes) { sV = s; sT = s; }
  const int ko = knockout_mask(e, true);
  const FrameGeom& g = e->geom;
  const size_t F = (size_t)f0;
  const int nCells = g.nFastCells;
  const bool fused = e->fused && g.fusedBlur && e->blurSpec == kBlurSpecCv4;  // the fused phase E implements spec 0 only
  PyramidViews pyr = {}, blur = {}, pyr0 = {}, blur0 = {};
  pyr.nlevels = blur.nlevels = pyr0.nlevels = blur0.nlevels = g.nlevels;
  pyr0.lv[0] = level0;
  for (int l = 0; l < g.nlevels; l++) {
    if (l > 0) pyr0.lv[l] = LevelView{e->d_pyr + g.lv[l].off, g.pyrBytes, g.lv[l].pitch, g.lv[l].w, g.lv[l].h};
    blur0.lv[l] = LevelView{e->d_blur + g.lv[l].off, g.pyrBytes, g.lv[l].pitch, g.lv[l].w, g.lv[l].h};
    pyr.lv[l] = pyr0.lv[l];
    pyr.lv[l].base += F * pyr0.lv[l].frameStride;
    blur.lv[l] = blur0.lv[l];
    blur.lv[l].base += F * blur0.lv[l].frameStride;
  }
  if (e->copyUnaligned && ((level0.pitch & 3) || (level0.frameStride & 3) || (reinterpret_cast<uintptr_t>(level0.base) & 3))) {
    // caller-owned frames that are not dword-aligned (e.g. a tight 1241-byte stride).  Round 1 copied them into the
    // handle's own 64-B pitched level-0 slab first (an extra read + write of every input pixel); since round 2 the
    // four consumers of level 0 (resize, FAST, blur, orientation) read byte-aligned requests in place and the copy
    // is only kept behind $ORBFE_COPY_UNALIGNED=1 as a cross-check
    LevelView own{e->d_pyr + g.lv[0].off, g.pyrBytes, g.lv[0].pitch, g.lv[0].w, g.lv[0].h};
    LevelView src = level0;
    src.base += F * level0.frameStride;
    LevelViewMut dst{e->d_pyr + g.lv[0].off + F * g.pyrBytes, g.pyrBytes, g.lv[0].pitch, g.lv[0].w, g.lv[0].h};
    launch_copy2d(s, src, dst, nFrames);
    pyr0.lv[0] = own;
    pyr.lv[0] = own;
    pyr.lv[0].base += F * own.frameStride;
  }
  if (pyrOut) { *pyrOut = pyr0; *blurOut = blur0; }
  // level l of this sub-batch's slice of the handle's own pyramid / blurred slab, writable
  auto mut = [&](const PyramidViews& v, int l) {
    return LevelViewMut{const_cast<uint8_t*>(v.lv[l].base), g.pyrBytes, g.lv[l].pitch, g.lv[l].w, g.lv[l].h};
  };
  Candidate* slots = e->d_slots + F * g.totalSlots;
  Candidate* cand = e->d_cand + F * g.totalSlots;
  uint16_t* cellCount = e->d_cellCount + F * nCells;
  int32_t* cellPrefix = e->d_cellPrefix + F * nCells;
  int32_t* candCount = e->d_candCount + F * g.nlevels;
  LevelKp* levelKp = e->d_levelKp + F * g.totalKpCap;
  int32_t* levelCount = e->d_levelCount + F * g.nlevels;
  // pyrBlur: level l is blurred and level l+1 written by ONE kernel per level (the staged tile serves both), so the
  // separate blur launch below is skipped; needs the packed resize tables and the unfused FAST kernel
  // (not for the few-frame launches of a live camera: there the 8 dependent blur + resize launches are a longer critical
  // path than 7 small resize launches followed by one blur launch -- 0.195 vs 0.167 ms per single frame)
  const bool pyrBlur = e->pyrBlur && !fused && !lanes && nFrames > 8;
  // a few frames (the live camera): the whole pyramid in ONE launch -- every tile recomputes its chain from level 0 in LDS
  // (k_pyramid_chain) -- instead of n-1 dependent launches of a few microseconds each
  const bool chain = e->pyrChain && e->chainOk && !pyrBlur && !fused && nFrames <= 8 && !(ko & 1);
  if (chain) {
    StageTimer t(e, ORBFE_STAGE_PYRAMID, 1, nFrames, sub, s);
    PyrChainArgs ca = {};
    ca.l0 = pyr.lv[0];
    for (int l = 0; l < g.nlevels; l++) { ca.w[l] = g.lv[l].w; ca.h[l] = g.lv[l].h; }
    for (int l = 1; l < g.nlevels; l++) {
      ca.lv[l] = mut(pyr, l);
      ca.xofs[l] = e->d_xofs[l]; ca.alpha[l] = e->d_alpha[l]; ca.yofs[l] = e->d_yofs[l]; ca.beta[l] = e->d_beta[l];
    }
    ca.tiles = e->d_chainTiles;
    ca.bufA = e->chainBufA; ca.bufB = e->chainBufB; ca.maxW = e->chainMaxW; ca.maxH = e->chainMaxH;
    launch_pyramid_chain(s, ca, e->nChainTiles, nFrames);
  } else
  {  // ComputePyramid, :1203-1234
    StageTimer t(e, ORBFE_STAGE_PYRAMID, pyrBlur ? g.nlevels : g.nlevels - 1, nFrames, sub, s);
    for (int l = 1; l <= g.nlevels && !(ko & 1); l++) {
      if (pyrBlur) {
        const LevelViewMut bdst = mut(blur, l - 1);
        if (l < g.nlevels && e->d_tileGx[l]) {
          launch_blur7_resize(s, pyr.lv[l - 1], bdst, mut(pyr, l), e->d_colrec[l], e->d_rowrec[l], e->d_tileGx[l], e->d_tileDy[l],
                              nFrames, e->blurSpec);
          continue;
        }
        launch_blur7(s, pyr.lv[l - 1], bdst, nFrames, e->blurSpec);
      }
      if (l == g.nlevels) break;
      launch_resize(s, pyr.lv[l - 1], mut(pyr, l), e->d_xofs[l], e->d_alpha[l], e->d_yofs[l], e->d_beta[l], e->d_colrec[l],
                    e->d_rowrec[l], nFrames);
    }
  }
  // GaussianBlur of every level, :1169-1175 -- the levels are independent: one launch.  It only needs
  // the pyramid, so odd sub-batches run it BEFORE the FAST stage: neighbouring streams are then in
  // different phases (VALU-bound blur/FAST next to latency-bound octree/descriptors) instead of in step.
  if (lanes) {
    HIPCHK(hipEventRecord(e->evPyr[sub], s));
    HIPCHK(hipStreamWaitEvent(sV, e->evPyr[sub], 0));
  }
  auto do_blur = [&]() {
    StageTimer t(e, ORBFE_STAGE_BLUR, 1, nFrames, sub, sV);
    LevelViewMut dsts[kMaxLevels];
    for (int l = 0; l < g.nlevels; l++)
      dsts[l] = mut(blur, l);
    launch_blur7_levels(sV, pyr.lv, dsts, g.nlevels, nFrames, e->blurSpec);
  };
  const bool blurFirst = !lanes && !fused && !pyrBlur && (sub & 1) != 0;  // measured +1.7 % frames/s (A/B on one box, 4 runs each)
  if (blurFirst) do_blur();
  {  // FAST grid stage, :846-896; fused: the same wavefronts also write the blurred level (:1169-1175)
    // threshold order: results are identical either way; auto follows the fallback rate of the launches that have
    // finished (hysteresis 0.40 / 0.50), so the choice lags the content by a call or two -- speed only
    if (e->fastMode == 0) {
      for (int i = 0; i < orbfe_extractor::kMaxStreams; i++)
        if (e->statPending[i] && hipEventQuery(e->evStat[i]) == hipSuccess) {
          e->statPending[i] = false;
          double hits = 0;
          for (int k = 0; k < orbfe_extractor::kStatSlots; k++) hits += e->h_fastStat[i * orbfe_extractor::kStatSlots + k];
          const double rate = e->statCells[i] > 0 ? 8.0 * hits / e->statCells[i] : 0.0;  // every 8th cell reports
          if (rate > 0.50) e->fastLowFirst = true;
          else if (rate < 0.40) e->fastLowFirst = false;
        }
      (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is not an error
    }
    const bool lowFirst = e->fastMode == 2 || (e->fastMode == 0 && e->fastLowFirst);
    unsigned int* stat = nullptr;
    // (not for the few-frame launches of a live camera: the two tiny copies and the event cost ~10 us of latency there)
    if (e->fastMode == 0 && nFrames > 8 && sub >= 0 && sub < orbfe_extractor::kMaxStreams && !e->statPending[sub]) {
      stat = e->d_fastStat + sub * orbfe_extractor::kStatSlots;
      HIPCHK(hipMemsetAsync(stat, 0, sizeof(unsigned int) * orbfe_extractor::kStatSlots, sV));
    }
    if (!(ko & 2)) {
      StageTimer t(e, ORBFE_STAGE_FAST, 1, nFrames, sub, sV);
      launch_fast_cells(sV, pyr, e->d_cells, nCells, nFrames, e->tab.iniThFAST, e->tab.minThFAST, slots, g.totalSlots,
                        cellCount, g.maxCellW, g.maxCellH, fused ? &blur : nullptr, (int)g.cells.size(), lowFirst, stat);
    }
    if (stat) {
      HIPCHK(hipMemcpyAsync(e->h_fastStat + sub * orbfe_extractor::kStatSlots, stat, sizeof(unsigned int) * orbfe_extractor::kStatSlots,
                            hipMemcpyDeviceToHost, sV));
      HIPCHK(hipEventRecord(e->evStat[sub], sV));
      e->statPending[sub] = true;
      e->statCells[sub] = (double)nCells * nFrames;
    }
  }
  if (lanes) {  // the tail lane starts on the candidates while the VALU lane goes on with the blur
    HIPCHK(hipEventRecord(e->evFast[sub], sV));
    HIPCHK(hipStreamWaitEvent(sT, e->evFast[sub], 0));
    if (!fused && !pyrBlur) do_blur();
    HIPCHK(hipEventRecord(e->evBlur[sub], sV));
  }
  if (ko & 4) {
  } else if (!e->hostOctree) {  // candidate ordering + DistributeOctTree, :566-808, one workgroup per (frame, level)
    // (round 4, measured and not kept: the candidate ordering INSIDE the octree kernel, in front of each (frame, level) item --
    // one launch and one global round trip fewer per chain; KITTI 100.6 k vs 101.4 k, TUM 361.9 k vs 360.1 k stereo frames /
    // frames per second for separate vs fused in a same-box A/B: the launch is not what the chain waits for)
    StageTimer t(e, ORBFE_STAGE_OCTREE, 2, nFrames, sub, sT);
    const bool octGathers = octree_gathers(nFrames, e->octreeMaxL);  // a few frames: the octree workgroups gather their own level
    if (!octGathers)
      launch_gather_candidates(sT, e->d_cells, e->d_lvgeom, g.nlevels, nFrames, slots, g.totalSlots, cellCount,
                               nCells, cand, candCount, cellPrefix);
    OctreeArgs oa = {};
    if (octGathers) {
      oa.gCells = e->d_cells; oa.gSlots = slots; oa.gCellCount = cellCount; oa.gCellsPerFrame = nCells; oa.gCellPrefix = cellPrefix;
      oa.gCand = cand; oa.gCandCount = candCount;
    }
    oa.cand = cand;
    oa.slotsPerFrame = g.totalSlots;
    oa.candCount = candCount;
    oa.lvg = e->d_lvgeom;
    oa.nlevels = g.nlevels;
    oa.nodeOf = e->d_nodeOf + F * g.totalSlots;
    oa.levelKp = levelKp;
    oa.levelCount = levelCount;
    oa.kpSlotsPerFrame = g.totalKpCap;
    oa.maxL = e->octreeMaxL;
    oa.narrowLevels = octree_narrow_levels(g.lv, g.nlevels);
    oa.work = e->d_octreeWork ? e->d_octreeWork + F * (size_t)g.nlevels * e->octreeWorkStride : nullptr;
    oa.workStride = e->octreeWorkStride;
    HIPCHK(launch_octree(sT, oa, g.nlevels, nFrames));
  } else {
    launch_gather_candidates(s, e->d_cells, e->d_lvgeom, g.nlevels, nFrames, slots, g.totalSlots, cellCount,
                             nCells, cand, candCount, cellPrefix);
    int rc = run_host_octree(e, nFrames);  // single-stream debug path: f0 == 0
    if (rc) return rc;
  }
  if (!lanes && !blurFirst && !fused && !pyrBlur) do_blur();
  if (lanes) HIPCHK(hipStreamWaitEvent(sT, e->evBlur[sub], 0));

  if (!(ko & 8)) {  // computeOrientation + computeDescriptors + output records
    StageTimer t(e, ORBFE_STAGE_ORIENT_DESC, 1, nFrames, sub, sT);
    OrientDescArgs a = {};
    a.pyr = pyr;
    a.blur = blur;
    a.nlevels = g.nlevels;
    a.kpSlotsPerFrame = g.totalKpCap;
    a.outCapacity = capacity;
    for (int l = 0; l < g.nlevels; l++) {
      a.kpStart[l] = g.lv[l].kpStart;
      a.kpCap[l] = g.lv[l].kpCap;
      a.scale[l] = e->tab.scale[l];
      a.kpSize[l] = (float)(int)(kPatchSize * e->tab.scale[l]);  // :905
    }
    // Tile form (k_desc_tiles.hip, round 3): a third of the HBM / L2 traffic of the per-keypoint gathers, but 1.6x their
    // VALU instructions (every tile pays its staging and list scan for ~19 keypoints) -- on this instruction-bound
    // pipeline it measures 2 % slower, so it is an option (orbfe_extractor_set_desc_tiles / $ORBFE_DESC_TILES=1), not
    // the default; DESIGN.md 4 has the counters.
    static const int kTilesEnv = getenv("ORBFE_DESC_TILES") ? atoi(getenv("ORBFE_DESC_TILES")) : 0;
    const int tilesMode = e->descTilesMode >= 0 ? e->descTilesMode : kTilesEnv;
    if (tilesMode && e->nDescTiles > 0)
      launch_orient_desc_tiles(sT, a, e->d_descTiles, e->nDescTiles, levelKp, levelCount, e->d_patternF, e->d_momentTab,
                               e->d_umax, nFrames, d_kp + F * capacity, d_desc + F * (size_t)capacity * 32, d_nOut + F, e->last.S);
    else
      launch_orient_desc(sT, a, levelKp, levelCount, e->d_patternF, e->d_momentTab, e->d_umax, nFrames,
                         d_kp + F * capacity, d_desc + F * (size_t)capacity * 32, d_nOut + F, e->last.S);
  }
  if (lanes) {
    HIPCHK(hipEventRecord(e->evTail[sub], sT));
    e->tailPending[sub] = true;
  }
  HIPCHK(hipGetLastError());
  return ORBFE_OK;
}

// One call = up to nStreams sub-batches of consecutive frames, each on its own HIP stream with
// its own slice of the workspace: the VALU-bound kernels (FAST, blur) of one sub-batch overlap the
// gather/latency-bound ones (orientation+descriptor, octree, resize) of the other.
int orbfe::run_pipeline(orbfe_extractor* e, LevelView level0, int nFrames, orbfe_keypoint* d_kp,
                        uint8_t* d_desc, int capacity, int32_t* d_nOut, const hipEvent_t* waitFor, int nWait,
                        const PreChunk* pre) {
  SubSplit sp;
  sp.frames = nFrames;
  sp.S = e->hostOctree ? 1 : e->nStreams;
  if (sp.S > nFrames) sp.S = nFrames;
  if (sp.S < 1) sp.S = 1;
  sp.per = (nFrames + sp.S - 1) / sp.S;
  if ((nFrames & 1) == 0 && (sp.per & 1)) sp.per++;  // stereo batches (L0,R0,L1,R1,...): never split a pair across sub-batches
  sp.lanes = e->laneMode && !e->hostOctree && sp.S >= 2;
  e->haveLast = false;  // (until this call is enqueued in full)
  if (!(sp == e->last)) {
    // a different split maps frames to different streams: drain everything first
    int rcs = sync_all(e);
    if (rcs) return rcs;
    e->last = sp;
  }
  // a frame build still reading the output block this call overwrites: every stream that writes the block waits for it
  // (stream 0 included -- the build runs on another thread's matcher stream)
  if (e->readerPending) {
    if (hipEventQuery(e->evReaderDone) == hipSuccess) e->readerPending = false;
    (void)hipGetLastError();  // hipEventQuery's hipErrorNotReady is not an error
  }
  const bool readerWait = e->readerPending && d_kp == e->d_kpOut;
  hipStream_t sP = nullptr, sV = nullptr, sT = nullptr;
  if (sp.lanes) {
    sP = e->extra[0]; sV = e->extra[1]; sT = e->stream;
    if (e->consumerPending) HIPCHK(hipStreamWaitEvent(sP, e->evConsumerDone, 0));  // a matcher still reads the last pyramid
    if (readerWait) HIPCHK(hipStreamWaitEvent(sP, e->evReaderDone, 0));  // (V and T start behind P's events)
    for (int k = 0; k < nWait; k++) {  // e.g. the H2D copy of this chunk (read by P, V and T), the D2H of its output block (T)
      HIPCHK(hipStreamWaitEvent(sP, waitFor[k], 0));
      HIPCHK(hipStreamWaitEvent(sT, waitFor[k], 0));
    }
  } else {
    for (int i = 0; i < orbfe_extractor::kMaxStreams; i++) e->tailPending[i] = false;  // (drained above if the mode changed)
  }
  int f0, n;
  for (int i = 0; sp.range(i, &f0, &n); i++) {
    hipStream_t s = sp.lanes ? sP : (i == 0 ? e->stream : e->extra[i - 1]);  // the stream sub-batch i starts on
    if (sp.lanes) {
      // slice i of the workspace is free once the previous call's tail lane has finished with it
      // (slice i's readers of the previous call: behind evTail[i] / evConsumerDone, waited for above)
      if (e->tailPending[i]) HIPCHK(hipStreamWaitEvent(sP, e->evTail[i], 0));
    } else {
      if (i > 0 && e->consumerPending) HIPCHK(hipStreamWaitEvent(s, e->evConsumerDone, 0));
      if (readerWait) HIPCHK(hipStreamWaitEvent(s, e->evReaderDone, 0));
      for (int k = 0; k < nWait; k++) HIPCHK(hipStreamWaitEvent(s, waitFor[k], 0));  // e.g. the H2D copy of this chunk
    }
    if (pre && pre->fn) {
      StageTimer t(e, ORBFE_STAGE_H2D, 2, n, i, s);  // "h2d" = the ingest stage of a call: here the rectification
      int rcp = pre->fn(pre->ctx, s, f0, n);
      if (rcp) return rcp;
    }
    int rc = run_chunk(e, s, i, level0, f0, n, d_kp, d_desc, capacity, d_nOut, i == 0 ? &e->lastPyr : nullptr,
                       i == 0 ? &e->lastBlur : nullptr, sV, sT);
    if (rc) return rc;
    if (!sp.lanes && i > 0) HIPCHK(hipEventRecord(e->evChunkDone[i], s));
  }
  // lanes: every sub-batch ends on `stream`, so consumers there are ordered behind all of them; otherwise stream 0 is
  // ordered behind the consumer by itself and joins the others through evChunkDone
  e->consumerPending = false;
  e->chunksPending = sp.lanes ? 1 : sp.S;
  e->lastFrameBase = 0;
  e->haveLast = true;
  return ORBFE_OK;
}

// The prologue of every extract call: the output block is forgotten, geometry and a workspace for nFrames exist, the
// stage timers have a ring slot.  drain: the call starts on an idle handle (the host-buffer calls); otherwise the handle
// is only drained when the workspace is about to be re-allocated.
int orbfe::begin_call(orbfe_extractor* e, int W, int H, int nFrames, bool drain) {
  HIPCHK(hipSetDevice(e->device));
  int rc;
  if (drain || e->geom.W != W || e->geom.H != H || nFrames > e->capFrames)
    if ((rc = sync_all(e))) return rc;
  e->outLastFrames = 0;  // "the frame this handle produced last" is no longer the one in its own output block
  if ((rc = ensure_geometry(e, W, H))) return rc;
  if ((rc = ensure_workspace(e, nFrames))) return rc;
  next_event_slot(e);
  return ORBFE_OK;
}
