// match_kernels.h -- argument blocks of the matching kernels (k_match.hip).
#pragma once
#include <stdint.h>

#include "../../include/orbfe.h"
#include "kernels.h"

namespace orbfe {

struct NodePair {  // one vocabulary node present in both FeatureVectors
  int32_t off1, cnt1, off2, cnt2;
};

struct BowArgs {
  const NodePair* pairs;
  const uint8_t* desc1; const uint8_t* hasMp1 /* NULL: all set */; const float* angle1; const uint32_t* indices1;
  const uint8_t* desc2; const uint8_t* hasMp2 /* NULL for the KF-Frame form */; const float* angle2;
  const uint32_t* indices2;
  int angleStride;  // floats between consecutive angles (1 for plain arrays, 7 inside cv::KeyPoint records)
  float nnratio;
  int strictLow;   // 0: SearchByBoW(KF,F) accepts best <= TH_LOW; 1: (KF,KF) best < TH_LOW
  int32_t* match;  // KF-Frame: indexed by frame feature; KF-KF: indexed by KF1 feature
  int8_t* bin;     // rotation-histogram bin of the accepted match, same indexing
};

struct TriQuery { uint32_t idx1; int32_t off2, cnt2; };

struct TriArgs {
  const TriQuery* queries; int nQueries;
  const uint8_t* desc1; const float* x1; const float* y1; const float* angle1; const uint8_t* stereo1;
  const uint8_t* desc2; const uint8_t* hasMp2; const float* x2; const float* y2; const float* angle2;
  const int32_t* octave2; const uint8_t* stereo2; const uint32_t* indices2;
  const float* F12; float ex, ey;
  const float* scaleFactors2; const float* levelSigma2_2;
  int onlyStereo;
  int32_t* match; int8_t* bin;
};

struct StereoArgs {
  const float* kpL; const uint8_t* descL; int N;   // 7 floats per keypoint (cv::KeyPoint layout)
  const float* kpR; const uint8_t* descR; int Nr;
  PyramidViews pyrL, pyrR; int frameL, frameR;
  const float* scaleTab;  // device: mvScaleFactor[0..15] then mvInvScaleFactor[0..15]
  float mbf, maxD;
  float* uRight; float* depth; int32_t* sad;
  // optional row index of the right keypoints (NULL -> scan all): rows+1 starts and Nr indices per pair
  const int32_t* rowStart; const int32_t* sortedIdx; int rows; int bandR;
  // sortedRec[p] = (uR, yR, octave, iR) of the right keypoint at sorted position p (written by k_stereo_bucket next
  // to sortedIdx): the candidate scan reads ONE 16-byte record instead of the index and then three fields of the
  // 28-byte keypoint, i.e. one dependent memory round trip less per left keypoint
  const float4* sortedRec;
};

struct StereoBatch {  // frames 2p / 2p+1 of an extractor batch are the left / right image of pair p
  const float* kp; const uint8_t* desc; const int32_t* n; int capacity;
  float* uRight; float* depth; int32_t* sad;   // [nPairs * capacity]
};

// DBoW2 vocabulary tree on the device (vocabulary.hip; its kernels: k_vocab.hip).  Nodes are renumbered breadth-first so that the children of a
// node are ADJACENT records, in file order (the order TemplatedVocabulary::transform scans them in, :1236-1250): one
// level of the descent is one contiguous read of nChild x 48 bytes, and the record a lane loads to take its child's
// distance already carries what the next level needs if that child wins.
struct VocabNode {       // 48 bytes
  uint32_t d[8];         // FORB descriptor
  uint32_t firstChild;   // BFS position of the first child
  uint32_t nChild;       // bits 0-7: number of children (0 = leaf); bit 8: weight > 0
  uint32_t id;           // NodeId of the reference = line order of the text file (root = 0)
  int32_t word;          // WordId (leaves, in file order) or -1
};
struct VocabDevice {
  const VocabNode* nodes;  // [nNodes], BFS order, root at 0
  const double* weight;    // [nNodes], by BFS position
  uint32_t rootChildren;   // children of the root (positions 1 .. rootChildren)
};

// Batched FeatureVector construction: frame f uses desc[f*capacity ..], n[f] descriptors
struct FeatVecBatch {
  const uint8_t* desc; const int32_t* n; int capacity;
  int frameStep;             // frame f reads slot f*frameStep of desc / n (2: the left frames of an L,R-interleaved batch); 0 = 1
  int sortN;                 // power of two >= capacity
  uint32_t* word; double* weight;          // optional per-feature outputs [nFrames*capacity]
  unsigned long long* keys;  // [nFrames*capacity] scratch: (node << 32 | feature) of the used features, ~0 otherwise
  uint32_t* fvNodes;         // [nFrames*capacity] node ids ascending
  int32_t* fvOffsets;        // [nFrames*(capacity+1)]
  uint32_t* fvIndices;       // [nFrames*capacity]
  int32_t* fvCount;          // [nFrames] nodes per frame
};
void launch_vocab_featvec(hipStream_t s, const VocabDevice& v, const FeatVecBatch& b, int nFrames, int nidLevel);
// the descent alone (k_vocab.hip): descriptors [0, nPerFrame[f]) -- nPerFrame NULL: [0, nFixed) -- of every frame; word /
// weight / node / keys each optional
void launch_vocab_transform(hipStream_t s, const VocabDevice& v, const uint8_t* desc, const int32_t* nPerFrame, int nFixed,
                            int capacity, int frameStep, int nFrames, int nidLevel, uint32_t* word, double* weight, uint32_t* node,
                            unsigned long long* keys);

struct BowBatch {  // consecutive-frame SearchByBoW over a device-resident batch
  const float* kp; const uint8_t* desc; int capacity;
  int frameStep;             // frame p reads slot p*frameStep of kp / desc (as FeatVecBatch); 0 = 1
  const uint32_t* fvNodes; const int32_t* fvOffsets; const uint32_t* fvIndices; const int32_t* fvCount;
  float nnratio;
  int32_t* match; int8_t* bin;  // [nPairs*capacity], match pre-set to -1
};

// Frame grid + window search (k_window.hip)
constexpr int GRID_MAX_FEATURES = 16384;  // keys carry a 16-bit index and are sorted in 64 KB of LDS
struct GridFrame {
  const float* x; const float* y; const int32_t* octave; const float* uRight /* NULL: monocular */;
  const uint8_t* desc; int n;
  float minX, minY, wInv, hInv;  // mnMinX, mnMinY, mfGridElementWidthInv, mfGridElementHeightInv
};
struct WindowQueries {
  const float* x; const float* y; const float* r; const int32_t* minLevel; const int32_t* maxLevel;
  const uint8_t* active /* NULL: all */; const float* ur /* NULL: no stereo check */;
  const uint8_t* desc /* NULL: indices only */; int n; int K;
  // BEST mode (best != NULL; Fuse x2 / SearchBySim3, src/ORBmatcher.cc:1029-1075, 1217-1260): no list leaves the device --
  // per query the keypoint with the smallest distance in scan order (first minimum), optionally behind Fuse's chi-square
  // gate (gateUr = the projected ur of every query, invSigma2 = mvInvLevelSigma2), kept when its distance <= maxDist
  int32_t* best; const float* gateUr; const float* invSigma2; int gate; int maxDist;
};
// The claim loops of the projection searches on the device (k_window_claim): the reference walks its map points / key points
// IN ORDER and a point that takes a feature hides it from the later ones (src/ORBmatcher.cc:77-78, 1572-1574, 1726-1727,
// 431-432, 492-493).  One workgroup per job iterates "every query chooses among the features no EARLIER query holds" to its
// fixed point -- which is the sequential result (query 0's choice is final after round 1, query 1's after round 2, ...; in
// practice 2-3 rounds) -- so the candidate lists never leave the device: the match array comes back instead.
enum { CLAIM_BEST = 0, CLAIM_RATIO = 1, CLAIM_INIT = 2 };
struct ClaimJob {
  const int32_t* count; const uint32_t* cand;  // k_window_search's lists: (dist << 16 | feature) in scan order
  int K, nq, n;                 // list capacity, queries, features of the frame
  const uint8_t* active;        // [nq] NULL: every query takes part
  const uint8_t* blocked;       // [n] features that are taken at entry, NULL: none
  const uint8_t* blockVal;      // [nq] whether query i's match hides its feature (MapPoint::Observations() > 0), NULL: always
  const int32_t* octave;        // [n] (CLAIM_RATIO: the best / second-best level test, src/ORBmatcher.cc:100-127)
  const float* qAngle; const float* fAngle;  // rotation histogram (checkOri)
  const float* fx; const float* fy; const float* qx; const float* qy;  // CLAIM_INIT: "update prev matched" (:595-600):
  float* prevX; float* prevY;   // out [nq]: the matched feature's position, else the query's own
  int mode, maxDist, checkOri;
  float nnratio;
  int32_t* choice;  // [nq] scratch: the query's current choice (feature, or dist << 16 | feature in CLAIM_INIT), -1 none
  int32_t* link;    // [nq] scratch (CLAIM_INIT: the other queries that chose the same feature)
  int32_t* owner;   // [2 n] ([n] for CLAIM_INIT) scratch in HBM, NULL: the kernel's dynamic LDS holds it
  int32_t* match;   // out.  BEST / RATIO: [n], query that holds feature i or -1.  INIT: [nq], feature of query i or -1
  int32_t* header;  // out [4]: largest list length (> K: the lists were truncated, search again), matches, rounds, 0
};
void launch_window_claim(hipStream_t s, const ClaimJob* d_jobs, const ClaimJob* h_first /* host copy of job 0 */, int nJobs, size_t ldsBytes,
                         bool initForm /* all jobs CLAIM_INIT, or none */);
void launch_grid_build(hipStream_t s, const GridFrame& f, uint32_t* sortedKey, int32_t* cellOff);
void launch_frame_from_records(hipStream_t s, const float* d_kp, const uint8_t* d_desc, int n, float* x, float* y, float* angle,
                               int32_t* octave, uint8_t* descOut, uint8_t* stereoZero);
struct WindowSearchJob {  // one job of k_window_search_multi; blockStart = first workgroup of the job (4 queries per workgroup)
  GridFrame f; const uint32_t* sortedKey; const int32_t* cellOff; WindowQueries q; int32_t* count; uint32_t* cand; int blockStart;
};
void launch_window_search_multi(hipStream_t s, const WindowSearchJob* d_jobs, int nJobs, int totalBlocks);
void launch_window_search(hipStream_t s, const GridFrame& f, const uint32_t* sortedKey, const int32_t* cellOff,
                          const WindowQueries& q, int32_t* count, uint32_t* cand);

// Device map-point table (k_project.hip).  Slot s of the table: rec[2 s] = (X, Y, Z, mfMinDistance), rec[2 s + 1] = (nx, ny, nz,
// mfMaxDistance), desc[32 s ..], flags[s] (ORBFE_MP_BAD | ORBFE_MP_OBSERVED).
struct MapPointsDevice { float4* rec; uint8_t* desc; uint8_t* flags; };
// Where a prologue writes the queries of the window search (k_window.hip: WindowQueries), and what the host holds of a job's
// queries.  x == NULL: the launch writes no windows.  Optional, each NULL when nobody reads it: ur (the projected right
// coordinate: the stereo check, or Fuse's chi-square gate), obs (Observations() > 0: does the point's match hide its feature),
// validCopy (a second copy of `active` among the results that travel back).  desc rows are 32 bytes.
struct QueryOut {
  float* x; float* y; float* r; int32_t* minLevel; int32_t* maxLevel; uint8_t* active;
  float* ur; uint8_t* desc; uint8_t* obs; uint8_t* validCopy;
};
// k_project_frustum: Frame::isInFrustum + MapPoint::PredictScale (src/Frame.cc:292-353) for the n points slot[0 .. n), one
// lane per point.  Two sets of outputs, either may be absent: the fields isInFrustum leaves on the MapPoint (every pointer may
// be NULL), and -- q.x != NULL -- the query windows of SearchByProjection(Frame&, vector<MapPoint*>&, th) exactly as
// orbfe_search_by_projection builds them on the host (src/ORBmatcher.cc:51-76), with the points' descriptors gathered from
// the table, so that k_window_search / k_window_claim run behind it without a host step.
struct ProjectArgs {
  MapPointsDevice table;
  const int32_t* slot; const uint8_t* skip /* NULL: none */; int n;
  orbfe_camera_pose cam; float limit;
  uint8_t* inView; int32_t* level; float* viewCos; float* projX; float* projY; float* projXr; float* invZ; float* dist;
  QueryOut q;
  const float* scale; float th;
};
void launch_project_frustum(hipStream_t s, const ProjectArgs& a);
// k_project_fuse: the prologue of ORBmatcher::Fuse (src/ORBmatcher.cc:960-1006; the Sim3 overload :1135-1184) for the n points
// slot[0 .. n) against K key-frame poses in ONE launch.  A workgroup owns 256 consecutive points, reads each point's two
// records and flag byte once and walks the K poses, which it holds in LDS.  Arrays of results are [k * n + i].  Two sets of
// outputs, either may be absent: the projection itself (every pointer may be NULL), and -- q.x != NULL -- the query windows of
// orbfe_fuse_search_multi exactly as it builds them on the host (centre (u, v), radius th * scale[level], octaves
// [level - 1, level]), with the points' descriptors gathered once for all K jobs, so that k_window_search runs behind it
// without a host step.  rows != NULL: IsInKeyFrame (:965) from the observation graph -- a point whose row names kfSlot[k]
// among its meta.count live entries is rejected for pose k; a slot at or past pointCap has no row.
constexpr int kFuseMaxKeyFrames = 64;
struct ObsEntry;      // obsgraph_host.h
struct ObsPointMeta;
struct FuseArgs {
  MapPointsDevice table;
  const int32_t* slot; const uint8_t* skip /* [K * n], NULL: none */; int n, K;
  const orbfe_camera_pose* pose /* [K] */; const int32_t* kfSlot /* [K], read only with rows */;
  const ObsEntry* rows; const ObsPointMeta* meta; int rowWidth, pointCap;
  uint8_t* valid; float* u; float* v; float* ur; int32_t* level; float* dist;
  QueryOut q;  // (desc: [n * 32], once for all K)
  const float* scale; float th;
};
void launch_project_fuse(hipStream_t s, const FuseArgs& a);
// k_project_track: the prologues of the two tracking-thread searches that walk a frame's own map points, for K jobs over
// concatenated lists in ONE launch (blockIdx.y = job k, points [offsets[k], offsets[k + 1]), pose[k], th[k]); one lane per point.
//   form 0, SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1516-1550): no isBad test, invz < 0
//   rejected, radius th * scale[lastOctave], the level range of `mode` (0 / 1 bForward / 2 bBackward), q.obs = Observations() > 0;
//   form 1, SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (:1665-1699): isBad and skip rejected, no depth
//   sign test, the distance range, PredictScale, radius th * scale[level], levels [level - 1, level + 1].
// Two sets of outputs, either may be absent: the projection itself (every pointer may be NULL; entries of a rejected point
// are 0) and -- q.x != NULL -- the query windows exactly as orbfe_search_by_projection_last_frame / _keyframe build them on the
// host, with the points' descriptors gathered from the table, so that k_window_search / k_window_claim run behind it without
// a host step.  Every array is indexed by the position in the concatenated list.
constexpr int kTrackMaxJobs = 64;
struct TrackArgs {
  MapPointsDevice table;
  int form, K, mode;
  const int32_t* offsets /* [K + 1] */; const int32_t* slot; const uint8_t* skip /* NULL: none */;
  const int32_t* lastOctave /* form 0 */; const orbfe_camera_pose* pose /* [K] */; const float* th /* [K] */;
  uint8_t* valid; float* u; float* v; float* invZ; float* ur /* form 0 */; float* radius /* form 0 */;
  int32_t* level /* form 1 */; float* dist /* form 1 */;
  QueryOut q;  // (ur, obs: form 0)
  const float* scale;
};
void launch_project_track(hipStream_t s, const TrackArgs& a, int maxN /* the longest list of the K jobs */);
// k_project_sim3: the prologue of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1298-1340 and :1379-1420) for nLegs legs in ONE
// launch; a leg is one direction of one candidate (blockIdx.y = leg, one lane per point, a workgroup owns 256 consecutive
// points of its leg).  Leg l reads slot[span.slotOff + i] (-1: no map point) and writes every array at [span.outOff + i], so
// the K "1 -> 2" legs of a call share ONE copy of KF1's slot list and -- span.flags & 1 on the first of them only -- one gather
// of its descriptors into q.desc[(span.slotOff + i) * 32].  span.flags & 2: the leg's target uses the second level table
// (scale + nLevels).  Two sets of outputs, either may be absent, as for k_project_fuse; the arithmetic is include/orbfe.h's
// (orbfe_project_sim3), operation by operation.
constexpr int kSim3MaxLegs = 128;
struct Sim3Span { int32_t slotOff, n, outOff, flags; };
struct Sim3Args {
  MapPointsDevice table;
  int nLegs, nLevels;
  const Sim3Span* span /* [nLegs] */; const orbfe_sim3_leg* leg /* [nLegs] */;
  const int32_t* slot; const uint8_t* skip /* by output position, NULL: none */;
  uint8_t* valid; float* u; float* v; int32_t* level; float* dist;
  QueryOut q;  // (no ur, obs or validCopy; desc by slot position)
  const float* scale /* [nLevels] or [2 * nLevels] */; float th;
};
void launch_project_sim3(hipStream_t s, const Sim3Args& a, int maxN /* the longest leg */);
// vbAlreadyMatched2 of SearchBySim3 (:1282-1292) from the observation rows: for candidate k and keypoint i1 of KF1 with
// matched[k * n1 + i1] = slot s >= 0, the live entry of s's row whose kf == kfSlot[k] marks already2[offsets2[k] + idx] when
// idx < offsets2[k + 1] - offsets2[k] (MapPoint::GetIndexInKeyFrame); a slot at or past pointCap has no row.  Byte stores of 1.
void launch_sim3_already(hipStream_t s, const ObsEntry* rows, const ObsPointMeta* meta, int rowWidth, int pointCap, int K, int n1,
                         const int32_t* matched, const int32_t* kfSlot, const int32_t* offsets2, uint8_t* already2);
// orbfe_mappoints_update: n staged entries (slot, the two records, flags, descriptors or NULL = keep) into their slots
void launch_mappoints_scatter(hipStream_t s, const MapPointsDevice& t, int n, const int32_t* slot, const float4* rec,
                              const uint8_t* flags, const uint8_t* desc);
// the descriptors of slot[0 .. n) of a table into desc[n][32] (orbfe_mappoints_descriptors)
void launch_mappoints_read_descriptors(hipStream_t s, const MapPointsDevice& t, int n, const int32_t* slot, uint8_t* desc);

void launch_search_by_bow(hipStream_t s, const BowArgs& a, int nPairs, int maxCnt2);
void launch_search_by_bow_multi(hipStream_t s, const BowArgs* d_args, const int32_t* d_pairStart, int K, int nPairsTotal, int maxCnt2);
void launch_search_by_bow_batch(hipStream_t s, const BowBatch& b, int nPairs, int checkOri, int32_t* d_nMatches,
                                int maxNodes /* bound on FeatureVector entries per frame, 0: capacity */);
void launch_search_triangulation(hipStream_t s, const TriArgs& a);
void launch_search_triangulation_multi(hipStream_t s, const TriArgs* d_args, const int32_t* d_blockStart, int K, int totalBlocks);
void launch_rot_prune(hipStream_t s, int32_t* match, const int8_t* bin, int n, int checkOri, int32_t* nMatches);
void launch_rot_prune_batch(hipStream_t s, int32_t* match, const int8_t* bin, int n, int nArrays, int checkOri, int32_t* nMatches);
void launch_stereo(hipStream_t s, const StereoArgs& a, int32_t* d_nStereo);
void launch_stereo_batch(hipStream_t s, const StereoArgs& a, const StereoBatch& b, int nPairs, int32_t* d_nStereo);

}  // namespace orbfe
