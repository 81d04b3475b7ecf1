// extractor_handle.h -- struct orbfe_extractor and what the extractor's host files share (extractor_handle.hip: the handle,
// its streams, buffers and stage timers; extractor_pipeline.hip: the schedule of a call; extractor.hip: the extract calls and
// their host staging; stereo_batch.hip: the batched stereo matcher; extractor_debug.hip: the stall hooks).  No other host
// file includes it: they reach a handle through the back doors of host_internal.h.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "../../include/orbfe.h"
#include "host_internal.h"

// one timed interval of a stage (between the handle's events evA .. evB of the same index): what was launched in it
struct StageInterval {
  bool used = false;  // closed and not yet read out (resolve_slot)
  int launches = 0, frames = 0;
};

struct orbfe_extractor {
  orbfe::ExtractorTables tab;
  int device = 0;
  hipStream_t stream = nullptr;              // stream 0: owns the timing events and the copies
  static constexpr int kMaxStreams = 32;
  hipStream_t extra[kMaxStreams - 1] = {};   // sub-batch streams 1..31
  int nStreams = 1;                          // >1: sub-batches of one call run concurrently
  int subsReady = 0;                         // sub-batches whose stream and events exist (ensure_subs)
  // cross-stream ordering without host synchronisation: evChunkDone[i] marks the end of sub-batch i of the
  // last extract call (consumers on `stream` wait for it); evConsumerDone marks the end of the last kernel
  // on `stream` that READS the workspace / the caller's outputs of all sub-batches (batched stereo matcher),
  // and every sub-batch stream of the next extract call waits for it before it overwrites them
  // lane schedule (laneMode): every sub-batch uses the same three streams -- P = extra[0] (pyramid), V = extra[1]
  // (FAST, blur: the VALU-bound kernels), T = stream (gather, octree, orientation + descriptors: the latency-bound
  // tail) -- so the sub-batches form a software pipeline: while V works on sub-batch k, P already builds the pyramid
  // of k+1 and T finishes k-1.  One VALU-bound kernel is in flight at any time instead of whatever the phases of
  // independent sub-batch streams happen to overlap.  evPyr/evFast/evBlur order the lanes inside a sub-batch,
  // evTail[k] (end of sub-batch k on T) holds back the next call's pyramid of the same workspace slice.
  bool laneMode = false;
  hipEvent_t evPyr[kMaxStreams] = {}, evFast[kMaxStreams] = {}, evBlur[kMaxStreams] = {}, evTail[kMaxStreams] = {};
  bool tailPending[kMaxStreams] = {};
  hipEvent_t evChunkDone[kMaxStreams] = {};
  hipEvent_t evConsumerDone = nullptr;
  // a resident frame built from the output block (orbfe_frame_from_extractor) reads it on the building thread's matcher
  // stream: evReaderDone marks the end of that build, and the next call that writes the block waits for it (run_pipeline)
  hipEvent_t evReaderDone = nullptr;
  hipStream_t readerStream = nullptr;
  bool readerPending = false;
  int chunksPending = 0;                     // sub-batch streams 1..chunksPending-1 carry an unrecorded-for-consumer event
  bool consumerPending = false;
  orbfe::SubSplit last;           // how the last run_pipeline call was split
  double stageFrames[ORBFE_STAGE_COUNT] = {};
  // stage timing: a ring of event pairs per stage so that asynchronous calls can stay in flight
  static constexpr int kEvRing = 8;
  static constexpr int kEvSubs = kMaxStreams;  // one event pair per (call slot, sub-batch stream, stage)
  hipEvent_t evA[kEvRing][kEvSubs][ORBFE_STAGE_COUNT] = {}, evB[kEvRing][kEvSubs][ORBFE_STAGE_COUNT] = {};
  StageInterval ev[kEvRing][kEvSubs][ORBFE_STAGE_COUNT];
  int evSlot = 0;
  unsigned stageMask = 0;
  bool stage_on(int stage, int sub) const { return sub >= 0 && sub < kEvSubs && ((stageMask >> stage) & 1u); }
  // opens the interval of (stage, sub-batch) in the current ring slot on stream s -- or, when this slot already holds
  // one (a second matcher behind the same sub-batch: stereo, then BoW), counts the launches into it: one interval from
  // the first one's start to the last one's end
  void stage_open(int stage, int sub, hipStream_t s, int launches, int frames) {
    if (!stage_on(stage, sub)) return;
    StageInterval& iv = ev[evSlot][sub][stage];
    if (iv.used) { iv.launches += launches; return; }
    (void)hipEventRecord(evA[evSlot][sub][stage], s);
    iv.launches = launches;
    iv.frames = frames;
  }
  void stage_close(int stage, int sub, hipStream_t s) {
    if (!stage_on(stage, sub)) return;
    (void)hipEventRecord(evB[evSlot][sub][stage], s);
    ev[evSlot][sub][stage].used = true;
  }
  bool hostOctree = false;  // debug cross-check only (orbfe_extractor_debug_host_octree)
  // GaussianBlur inside the FAST kernel (k_fast_cells<.., true>) instead of the separate k_blur7 launch.  Measured
  // (r02, same box, 4096 VGA frames): fused 8.41 ms vs 5.28 + 3.26 ms for the two launches, pipeline 285.9 k vs
  // 291.8 k frames/s -- FAST already runs at the VALU issue ceiling, so the blur's instructions cost their full price
  // inside it; off by default, selectable ($ORBFE_FUSED=1 / orbfe_extractor_set_fused) and parity-tested
  bool fused = false;
  // FAST threshold order (k_fast_cells<.., kLowFirst>): 0 = auto (picked per call from the fallback rate the last
  // finished launch measured), 1 = iniThFAST first + per-cell fallback, 2 = one attempt at the lower threshold
  int fastMode = 0;
  bool fastLowFirst = false;                 // current choice in auto mode
  static constexpr int kStatSlots = 64;       // counters per sub-batch (k_fast_cells spreads its sampled reports over them)
  orbfe::DevBuf<unsigned int> d_fastStat;    // per sub-batch: sampled count of cells that needed minThFAST
  orbfe::PinBuf<unsigned int> h_fastStat;    // pinned copy
  hipEvent_t evStat[kMaxStreams] = {};
  bool statPending[kMaxStreams] = {};
  double statCells[kMaxStreams] = {};
  bool copyUnaligned = false;  // debug: repack caller-owned frames with an odd stride first (round-1 behaviour)
  int blurSpec = orbfe::kBlurSpecCv4;  // GaussianBlur arithmetic, orbfe_extractor_set_blur_spec / $ORBFE_BLUR_SPEC
  int octreeMaxL = 0;
  double stageMs[ORBFE_STAGE_COUNT] = {};
  int64_t stageLaunches[ORBFE_STAGE_COUNT] = {};

  orbfe::FrameGeom geom;
  int capFrames = 0;  // frames the workspace is sized for
  // constant device tables
  orbfe::DevBuf<float4> d_patternF;
  orbfe::DevBuf<uint4> d_momentTab;
  orbfe::DevBuf<uint8_t> d_hostIn;  // input slab of the small host-batch path (frames at the caller's pitch)
  size_t hostInBytes = 0;
  orbfe::DevBuf<orbfe::DescTile> d_descTiles;  // tile form of the orientation + descriptor stage (k_desc_tiles.hip)
  int nDescTiles = 0;
  int knockoutChunks = 0;
  int descTilesMode = -1;           // -1: $ORBFE_DESC_TILES (default 0 = the per-keypoint form); 0 / 1 forced by orbfe_extractor_set_desc_tiles
  orbfe::DevBuf<int32_t> d_umax;
  orbfe::DevBuf<orbfe::CellDesc> d_cells;
  orbfe::DevBuf<orbfe::LevelGeom> d_lvgeom;
  orbfe::DevBuf<int32_t> d_xofs[orbfe::kMaxLevels];
  orbfe::DevBuf<int16_t> d_alpha[orbfe::kMaxLevels];
  orbfe::DevBuf<int32_t> d_yofs[orbfe::kMaxLevels];
  orbfe::DevBuf<int16_t> d_beta[orbfe::kMaxLevels];
  orbfe::DevBuf<uint32_t> d_colrec[orbfe::kMaxLevels];
  orbfe::DevBuf<uint32_t> d_rowrec[orbfe::kMaxLevels];
  orbfe::DevBuf<orbfe::ChainTile> d_chainTiles;  // the one-launch pyramid of the single-frame form (k_pyramid_chain): tiles + what each needs
  int nChainTiles = 0, chainBufA = 0, chainBufB = 0, chainMaxW = 0, chainMaxH = 0;
  bool chainOk = false;
  bool pyrChain = false;                // use it for calls of <= 8 frames ($ORBFE_PYR_CHAIN, orbfe_extractor_set_pyramid_chain): off,
                                        // it measured no faster than the seven launches
  orbfe::DevBuf<int32_t> d_tileGx[orbfe::kMaxLevels];  // ownership tables of the fused blur + resize kernel (ResizeTables::tileGx / tileDy)
  orbfe::DevBuf<int32_t> d_tileDy[orbfe::kMaxLevels];
  bool pyrBlur = true;                  // blur level l and write level l+1 from the same staged tiles ($ORBFE_PYRBLUR,
                                        // orbfe_extractor_set_pyramid_blur)
  // per-batch workspace
  orbfe::DevBuf<uint8_t> d_pyr;
  orbfe::DevBuf<uint8_t> d_blur;
  orbfe::DevBuf<orbfe::Candidate> d_slots;
  orbfe::DevBuf<orbfe::Candidate> d_cand;
  orbfe::DevBuf<uint16_t> d_cellCount;
  orbfe::DevBuf<int32_t> d_cellPrefix;
  orbfe::DevBuf<int32_t> d_candCount;
  orbfe::DevBuf<uint16_t> d_nodeOf;
  orbfe::DevBuf<uint8_t> d_octreeWork;  // node lists of k_octree_global (only when they do not fit in LDS)
  size_t octreeWorkStride = 0;
  orbfe::DevBuf<float> d_scaleTab;     // mvScaleFactor[16] + mvInvScaleFactor[16]
  orbfe::DevBuf<float> d_frameStereo;  // orbfe_extract_stereo_frame: mvuRight | mvDepth | survivors of the pair
  size_t frameStereoCap = 0;
  orbfe::DevBuf<int32_t> d_stereoSad;  // scratch of the batched stereo matcher
  orbfe::DevBuf<int32_t> d_stereoRowStart;
  orbfe::DevBuf<int32_t> d_stereoSorted;
  orbfe::DevBuf<float4> d_stereoRec;   // (uR, yR, octave, index) of the right keypoints in row order
  size_t stereoSadCap = 0, stereoRowCap = 0;
  orbfe::DevBuf<orbfe::LevelKp> d_levelKp;
  orbfe::DevBuf<int32_t> d_levelCount;
  // outputs of the host-buffer API: ONE block [keypoints | descriptors | counts], so a small batch
  // comes back in a single D2H copy through the pinned staging buffer
  orbfe::DevBuf<uint8_t> d_outBlock;
  orbfe_keypoint* d_kpOut = nullptr;
  uint8_t* d_descOut = nullptr;
  int32_t* d_nOut = nullptr;
  // the handle's own output block still holds the records of the last HOST-buffer call (orbfe_extract / small
  // orbfe_extract_batch): orbfe_frame_from_extractor builds resident frames from it without the features travelling again
  int outLastFrames = 0, outLastCapacity = 0;
  std::vector<int32_t> outLastCount;
  orbfe::PinBuf<uint8_t> h_outStage;
  size_t outStageBytes = 0;
  int outCap = 0;
  // pinned-host pipelined path (orbfe_extract_batch_pipelined): two input slabs + two output blocks in HBM,
  // one copy stream per direction, events per slot
  hipStream_t sH2D = nullptr, sD2H = nullptr;
  orbfe::DevBuf<uint8_t> d_pipeIn[2];
  orbfe::DevBuf<uint8_t> d_pipeOut[2];
  size_t pipeInBytes = 0, pipeOutBytes = 0;
  hipEvent_t evIn[2] = {}, evComp[2] = {}, evOutDone[2] = {};
  // host staging
  std::vector<int32_t> h_candCount, h_levelCount;
  std::vector<orbfe::Candidate> h_cand;
  std::vector<orbfe::LevelKp> h_levelKp;
  // description of the last call (for mvImagePyramid-style reads)
  orbfe::PyramidViews lastPyr = {};
  orbfe::PyramidViews lastBlur = {};
  int lastFrameBase = 0;  // index, in the caller's batch, of the first frame the retained pyramid belongs to (pipelined host path: its LAST chunk)
  bool haveLast = false;
};

namespace orbfe {

// Stage timing with HIP events on the handle's own stream.  Events are only RECORDED inside
// the pipeline (no host sync); resolve_stage_times() reads them after the call's final
// stream synchronisation, so profiling does not perturb the timed region.
struct StageTimer {
  orbfe_extractor* e;
  int stage, sub;
  hipStream_t s;
  // sub = index of the sub-batch (its stream is s); every sub-batch of a call is timed on its own stream
  StageTimer(orbfe_extractor* e_, int st, int n, int frames, int sub_, hipStream_t s_) : e(e_), stage(st), sub(sub_), s(s_) {
    e->stage_open(stage, sub, s, n, frames);
  }
  ~StageTimer() { e->stage_close(stage, sub, s); }
};

// `pre`: work enqueued on a sub-batch's stream in FRONT of its kernels (frames [f0, f0 + n) of the batch), e.g. the
// rectification that produces those frames -- stream order is the only synchronisation it needs, and what the previous
// call left on that stream (its kernels and matchers, which read the same frame slots) is behind it by construction.
struct PreChunk {
  int (*fn)(void* ctx, hipStream_t s, int f0, int n) = nullptr;
  void* ctx = nullptr;
};

// roles of the stream pool (stream_get): 0 = stream 0, i = sub-batch stream i, and the two copy streams
constexpr int kRoleH2D = 1000, kRoleD2H = 1001;

// ---- extractor_handle.hip ----
hipError_t stream_get(int device, int role, hipStream_t* s);
int ensure_geometry(orbfe_extractor* e, int W, int H);
int ensure_workspace(orbfe_extractor* e, int nFrames);
int ensure_outputs(orbfe_extractor* e, int nFrames, int capacity);
int sync_all(orbfe_extractor* e);
void resolve_stage_times(orbfe_extractor* e);
void next_event_slot(orbfe_extractor* e);
// ---- extractor_pipeline.hip ----
int knockout_mask(orbfe_extractor* e, bool count);
int run_pipeline(orbfe_extractor* e, LevelView level0, int nFrames, orbfe_keypoint* d_kp, uint8_t* d_desc, int capacity,
                 int32_t* d_nOut, const hipEvent_t* waitFor = nullptr, int nWait = 0, const PreChunk* pre = nullptr);
int begin_call(orbfe_extractor* e, int W, int H, int nFrames, bool drain);
// ---- extractor.hip ----
int ensure_host_in(orbfe_extractor* e, size_t bytes);
int fetch_outputs(orbfe_extractor* e, int nFrames, int capacity, orbfe_keypoint* const* kps, uint8_t* const* desc, int* n,
                  const void* d_tail = nullptr, size_t tailBytes = 0, const uint8_t** h_tail = nullptr);
int retained_frame(orbfe_extractor* e, int frame, int* local);

}  // namespace orbfe
