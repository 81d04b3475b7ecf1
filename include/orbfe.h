/*
 * orbfe.h -- C-ABI of the MI355X-native ORB front-end (liborbfe.so).
 *
 * Drop-in boundary for the ONE hot path of saber/ORB_SLAM2_Annotate:
 * ORBextractor::operator() + Hamming matchers + Frame::ComputeStereoMatches.
 * Plain pointers and sizes only; no C++/torch/OpenCV types; no exceptions cross
 * this boundary.  Every entry point cites the reference interface it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the thin C++
 * classes (include/ORBextractor.h, include/ORBmatcher.h of this repo) that keep
 * the reference's class API on top of these calls.
 *
 * Threading contract (reference: src/Frame.cc:78-81, src/LocalMapping.cc:261,
 * src/LoopClosing.cc:294): one extractor handle per thread, handles are fully
 * independent (own HIP stream + workspace); matcher entry points are re-entrant.
 *
 * There is NO CPU fallback: every call needs a gfx950 device and returns
 * ORBFE_ERR_HIP when the HIP runtime reports none.
 */
#ifndef ORBFE_H
#define ORBFE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ORBFE_MAX_LEVELS 16

enum {
  ORBFE_OK = 0,
  ORBFE_ERR_INVALID = -1,  /* bad argument (null pointer, non-positive size, ...) */
  ORBFE_ERR_CAPACITY = -2, /* caller-provided output buffer too small */
  ORBFE_ERR_HIP = -3,      /* HIP runtime / device failure (see orbfe_last_error) */
  ORBFE_ERR_NOMEM = -4
};

/* Layout-identical to cv::KeyPoint (28 bytes): pt.x, pt.y, size, angle, response,
 * octave, class_id -- what ORBextractor::operator() fills (src/ORBextractor.cc:905-916,1187-1195). */
typedef struct orbfe_keypoint {
  float x, y;
  float size;
  float angle;
  float response;
  int32_t octave;
  int32_t class_id;
} orbfe_keypoint;

typedef struct orbfe_extractor orbfe_extractor;

/* Thread-local text of the last failure (never NULL). */
const char *orbfe_last_error(void);
/* Number of visible HIP devices (0 if none / runtime error). */
int orbfe_device_count(void);

/* ------------------------------------------------------------------------- */
/* Extractor                                                                  */
/* ------------------------------------------------------------------------- */

/* Replaces ORBextractor::ORBextractor(int nfeatures, float scaleFactor, int nlevels,
 * int iniThFAST, int minThFAST)  (include/ORBextractor.h:52-53, src/ORBextractor.cc:415-486).
 * `device` = HIP device ordinal. */
int orbfe_extractor_create(int nfeatures, float scaleFactor, int nlevels, int iniThFAST,
                           int minThFAST, int device, orbfe_extractor **out);
void orbfe_extractor_destroy(orbfe_extractor *e);

/* GetLevels / GetScaleFactor / GetScaleFactors / GetInverseScaleFactors /
 * GetScaleSigmaSquares / GetInverseScaleSigmaSquares (include/ORBextractor.h:66-87).
 * Each `out` receives nlevels floats. */
int orbfe_extractor_get_levels(const orbfe_extractor *e);
float orbfe_extractor_get_scale_factor(const orbfe_extractor *e);
int orbfe_extractor_get_scale_factors(const orbfe_extractor *e, float *out);
int orbfe_extractor_get_inverse_scale_factors(const orbfe_extractor *e, float *out);
int orbfe_extractor_get_scale_sigma_squares(const orbfe_extractor *e, float *out);
int orbfe_extractor_get_inverse_scale_sigma_squares(const orbfe_extractor *e, float *out);
/* mnFeaturesPerLevel (src/ORBextractor.cc:448-458) and umax (:471-485), for tests. */
int orbfe_extractor_get_features_per_level(const orbfe_extractor *e, int32_t *out);
int orbfe_extractor_get_umax(const orbfe_extractor *e, int32_t *out16);
/* Upper bound on keypoints one frame can return (quota + octree overshoot, Appendix A3). */
int orbfe_extractor_max_keypoints(const orbfe_extractor *e);
/* Exact output bound for a width x height image: sum over levels of max(quota + 3, 4 * nIni), where
 * nIni = round(width' / height') roots start the octree (very wide, flat images can exceed the bound of
 * orbfe_extractor_max_keypoints, which assumes nIni <= 16). */
int orbfe_extractor_max_keypoints_for(const orbfe_extractor *e, int width, int height);

/* Replaces ORBextractor::operator()(InputArray image, InputArray mask (ignored),
 * vector<KeyPoint>&, OutputArray descriptors)  (src/ORBextractor.cc:1119-1197).
 * `image`: host, 8-bit single channel, row-major, `stride` bytes per row.
 * Writes up to `capacity` keypoints and capacity*32 descriptor bytes (row i <-> keypoint i);
 * *n_out = count.  Empty image (NULL or w/h<=0) -> ORBFE_OK with *n_out = 0
 * (the reference returns silently, :1122-1123). */
int orbfe_extract(orbfe_extractor *e, const uint8_t *image, int width, int height, int stride,
                  orbfe_keypoint *keypoints, uint8_t *descriptors, int capacity, int *n_out);

/* Batched form of the same call for n_frames equally-sized frames (frame f starts at
 * images + f*frame_stride).  Per-frame outputs are packed at fixed slots of
 * `capacity` entries: keypoints[f*capacity + i], descriptors[(f*capacity + i)*32];
 * n_out[f] = count of frame f.  This is how a stereo Frame (2 images, src/Frame.cc:78-81)
 * or a whole sequence shard is pushed through the GPU in one pass. */
int orbfe_extract_batch(orbfe_extractor *e, const uint8_t *images, int n_frames, int width,
                        int height, int stride, size_t frame_stride, orbfe_keypoint *keypoints,
                        uint8_t *descriptors, int capacity, int *n_out);

/* Pinned (page-locked) host memory for the buffers of orbfe_extract_batch_pipelined. */
int orbfe_host_alloc(void **p, size_t bytes);
void orbfe_host_free(void *p);

/* operator() for a host batch, end to end and pipelined: the batch is cut into chunks of chunk_frames (0 = 256); the
 * H2D copy of chunk k+1, the kernels of chunk k and the D2H copy of chunk k-1 overlap on separate HIP streams (two
 * input slabs / output blocks in HBM, ordered by events, no host wait inside the loop).  Output layout as
 * orbfe_extract_batch (frame f at keypoints + f*capacity, descriptors + f*capacity*32; rows past n_out[f] are
 * unspecified).  Buffers from orbfe_host_alloc move at PCIe speed; other memory is page-locked for the call. */
int orbfe_extract_batch_pipelined(orbfe_extractor *e, const uint8_t *images, int n_frames, int width, int height,
                                  int stride, size_t frame_stride, orbfe_keypoint *keypoints,
                                  uint8_t *descriptors, int capacity, int *n_out, int chunk_frames);

/* Same, but `d_images`, `d_keypoints`, `d_descriptors`, `d_n_out` are DEVICE pointers
 * (HBM-resident in, HBM-resident out; nothing crosses PCIe except per-batch control words).
 * The call returns after the work is complete on the handle's stream.
 * Frames are read IN PLACE at any stride and alignment; the kernels stage whole rows with 16-byte requests bounded by
 * the row PITCH, so every frame -- the last one included -- must be readable for stride * height bytes (a buffer that
 * ends at the last pixel of a frame with stride > width is not enough): frame_stride >= stride * height is required. */
int orbfe_extract_batch_device(orbfe_extractor *e, const uint8_t *d_images, int n_frames,
                               int width, int height, int stride, size_t frame_stride,
                               orbfe_keypoint *d_keypoints, uint8_t *d_descriptors, int capacity,
                               int32_t *d_n_out);

/* Asynchronous form: enqueues the whole batch on the handle's stream and returns; results are
 * valid after orbfe_extractor_synchronize (calls on one handle execute in order, so a caller may
 * keep several batches in flight as long as each uses its own output buffers). */
int orbfe_extract_batch_device_async(orbfe_extractor *e, const uint8_t *d_images, int n_frames,
                                     int width, int height, int stride, size_t frame_stride,
                                     orbfe_keypoint *d_keypoints, uint8_t *d_descriptors,
                                     int capacity, int32_t *d_n_out);
int orbfe_extractor_synchronize(orbfe_extractor *e);

/* Replaces reads of the public member `mvImagePyramid[level]` (include/ORBextractor.h:86;
 * read by Frame::ComputeStereoMatches, src/Frame.cc:519,609,621,626): copies level `level`
 * of frame `frame` of the LAST extract call into `dst` (host, dst_stride bytes per row).
 * level_size gives the dimensions for any input size.
 * `frame` always counts in the caller's batch.  The chunked host paths (orbfe_extract_batch_pipelined, and
 * orbfe_extract_batch when it routes a large batch there) keep the intermediate data of their LAST chunk only:
 * asking for a frame before it fails with ORBFE_ERR_INVALID ("pyramid of frame F not retained ...") -- this
 * holds for every frame-indexed accessor below and for orbfe_compute_stereo_matches. */
int orbfe_extractor_level_size(const orbfe_extractor *e, int width, int height, int level,
                               int *w, int *h);
int orbfe_extractor_get_pyramid_level(orbfe_extractor *e, int frame, int level, uint8_t *dst,
                                      int dst_stride);
/* Device view of the same (valid until the next extract call on this handle). */
int orbfe_extractor_pyramid_level_device(orbfe_extractor *e, int frame, int level,
                                         const uint8_t **d_ptr, int *pitch, int *w, int *h);

/* Stage diagnostics used by tests: raw grid-stage candidates of one level of frame 0 of
 * the last call, in emission order (src/ORBextractor.cc:846-896), coordinates relative to
 * (minBorderX,minBorderY).  Returns count or a negative status. */
int orbfe_extractor_debug_candidates(orbfe_extractor *e, int frame, int level, float *xs,
                                     float *ys, float *resp, int cap);
/* Blurred level (the `workingMat` of src/ORBextractor.cc:1169-1175) of the last call. */
int orbfe_extractor_debug_blurred_level(orbfe_extractor *e, int frame, int level, uint8_t *dst,
                                        int dst_stride);

/* Host-logic debug entry points; they run WITHOUT a GPU (CPU tests compare them with the oracle).
 * debug_octree_host: the library's host DistributeOctTree on flat arrays (candidates relative to
 * minBorder in emission order -> selected keypoints in list order, level coordinates); returns the count.
 * debug_geometry: per level 9 ints (w, h, nCols, nRows, wCell, hCell, nCells, quota, nIni) and the FAST
 * grid cells as 5 int16 (level, x0, y0, w, h: the detection rectangle); returns the cell count.
 * debug_resize_tables: the cv::resize fixed-point tables (xofs[dw], alpha[2*dw], yofs[dh], beta[2*dh]). */
int orbfe_debug_octree_host(const uint16_t *xs, const uint16_t *ys, const uint8_t *resp, int n, int minX, int maxX,
                            int minY, int maxY, int N, uint16_t *out_x, uint16_t *out_y, uint8_t *out_resp,
                            int cap);
/* debug_octree_device: DistributeOctTree of one DEVICE form on n_frames candidate sets of one distribution area -- the
 * operands of debug_octree_host (x, y relative to the area, 8-bit response, minX, maxX, minY, maxY, N), the sets
 * concatenated in xs / ys / resp with n_per_frame[f] candidates each.  The sets run as the (frame, level) items of ONE
 * launch of a one-level geometry; the candidates are handed over gathered (no in-kernel gather).  The host octree is
 * never called.
 *   form: 0 = the form the extractor's launch picks for n_frames frames, 1 = k_octree (throughput form: 16-bit counts, and
 *         k_octree_wide behind it for the sets of more than 65535 candidates), 2 = k_octree_reg,
 *         3 = k_octree_reg1024, 4 = k_octree_global.
 *   info6 (always written): nIni, kpCap (keypoint slots per frame), node capacity maxL, octree_lds_bytes(maxL), the LDS
 *         limit beyond which the node list lives in global memory, and the form that 0 stands for.  With out_x == NULL
 *         the call returns after writing it and needs no GPU.
 *   outputs, `cap` >= kpCap slots per frame (frame f at f * cap): every slot of the kernel's output array in the kernel's
 *         order -- spatial: 128-pixel column strip, then row, then column of the LEVEL coordinate x + 16, y + 16 -- with
 *         out_rank = the keypoint's position in the reference's list order; out_x / out_y are level coordinates
 *         (+ minX / + minY, as debug_octree_host).  out_count[f] keypoints are valid.  All scratch and output arrays are
 *         filled with 0xFF bytes before the launch and the kernels write nothing past a frame's count: the slots from
 *         out_count[f] to kpCap come back as 0xFFFF in all four arrays.
 * ORBFE_ERR_INVALID: form 1, 2 or 3 with a node list beyond the LDS limit (form 0 is then form 4).  Form 4 is accepted
 * at every size: k_octree_global needs nothing but its slab, which this entry allocates whenever form 4 runs. */
int orbfe_debug_octree_device(int device, int form, int n_frames, const uint16_t *xs, const uint16_t *ys,
                              const uint8_t *resp, const int32_t *n_per_frame, int minX, int maxX, int minY, int maxY,
                              int N, uint16_t *out_x, uint16_t *out_y, uint16_t *out_resp, uint16_t *out_rank,
                              int32_t *out_count, int cap, int32_t *info6);
/* debug_octree_carve (no GPU needed): how the octree kernels lay out the node arrays of one (frame, level) item of node
 * capacity maxL, with 16-bit counts (narrow != 0: k_octree) or 32-bit counts (every other kernel).
 *   out11: the byte offsets of rect[0], rect[1], cnt[0], cnt[1], child, scanA, scanB, order, inS; the end of the carve;
 *          and octree_lds_bytes(maxL, narrow), the LDS a launch asks for. */
int orbfe_debug_octree_carve(int maxL, int narrow, int64_t *out11);
int orbfe_debug_geometry(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int width,
                         int height, int32_t *levels9, float *tables4 /* scale, invScale, sigma2, invSigma2 per level; may be NULL */,
                         int16_t *cells5, int cell_cap);
int orbfe_debug_resize_tables(int sw, int sh, int dw, int dh, int32_t *xofs, int16_t *alpha, int32_t *yofs,
                              int16_t *beta);
/* Tile ownership of the fused blur + resize kernel for one level pair: tile_gx[(sw+63)/64 + 1] / tile_dy[(sh+63)/64 + 1]
 * (first 4-column group / output row owned by each 64 x 64 source tile, then the totals), group_start[(dw+3)/4] (first
 * source column of each group's 8-byte tap window), row_upper[dh] (upper source row of each output row, clamped).
 * *n_tiles_x / *n_tiles_y are 0 when the fused kernel is not used for these sizes. */
int orbfe_debug_resize_tiles(int sw, int sh, int dw, int dh, int32_t *tile_gx, int *n_tiles_x, int32_t *tile_dy,
                             int *n_tiles_y, int32_t *group_start, int32_t *row_upper);

/* Debug cross-check: when enabled, DistributeOctTree runs in the library's host implementation
 * (D2H/H2D round trip) instead of the device kernel.  Off by default; results are identical. */
int orbfe_extractor_debug_host_octree(orbfe_extractor *e, int enable);

/* Order of the two FAST thresholds inside the grid-stage kernel (src/ORBextractor.cc:874-882): 1 = iniThFAST first and
 * minThFAST only for the cells that found nothing (the reference's own order; fastest on textured images), 2 = one
 * attempt at the lower threshold that classifies for both (fastest when most cells fall back: sparse, low-contrast
 * images), 0 = auto (default; $ORBFE_FAST_MODE=auto|high|low): per call, from the fallback rate the last finished
 * launch measured.  The results are identical in every mode. */
int orbfe_extractor_set_fast_mode(orbfe_extractor *e, int mode);

/* Orientation + descriptor stage: 0 (default) = per-keypoint gathers (k_orient_desc), 1 = tile form (k_orient_desc_tiles:
 * a workgroup stages a 128 x 128 tile of the level and of the blurred level in LDS once for all keypoints inside it),
 * -1 = $ORBFE_DESC_TILES or the default.  Identical results; see DESIGN.md 4 for when which one is faster. */
int orbfe_extractor_set_desc_tiles(orbfe_extractor *e, int enable);
/* How the sub-batches of a device-batch call (orbfe_extractor_set_streams) are scheduled: 0 = one independent HIP
 * stream per sub-batch; 1 ($ORBFE_LANES) = three lanes shared by all sub-batches -- pyramid | FAST + blur |
 * gather + octree + orientation/descriptors -- ordered by events into a software pipeline, so that exactly one
 * VALU-bound kernel runs beside the latency-bound ones at any time.  Results are identical. */
int orbfe_extractor_set_schedule(orbfe_extractor *e, int lanes);

/* Which cv::GaussianBlur(7x7, sigma 2) arithmetic the extractor reproduces.  The reference does not pin its OpenCV
 * (CMakeLists.txt:33-39 accepts 2.4.3 and 3.x, README.md:74 names 2.4.11 / 3.2) and the 8-bit path changed:
 *   ORBFE_BLUR_CV4        (0, default; $ORBFE_BLUR_SPEC) OpenCV >= 3.4.1 / 4.x: taps 18 34 48 56 48 34 18 (/256),
 *                          (x + 2^15) >> 16;
 *   ORBFE_BLUR_CV2_SCALAR (1) OpenCV 2.4.x / 3.0-3.3 without SIMD: taps 18 34 49 55 49 34 18 (each rounded on its own,
 *                          sum 257), saturate((x + 2^15) >> 16);
 *   ORBFE_BLUR_CV2_SSE2   (2) the same versions on x86 with SSE2: round-half-to-even on the first width & ~3 columns
 *                          (float column pass + cvtps2dq), the scalar form on the last width & 3.
 * All three are restated from OpenCV's published sources and unverifiable in this image; the CPU
 * oracle implements the same three and the GPU equals it for each. */
enum { ORBFE_BLUR_CV4 = 0, ORBFE_BLUR_CV2_SCALAR = 1, ORBFE_BLUR_CV2_SSE2 = 2 };
int orbfe_extractor_set_blur_spec(orbfe_extractor *e, int spec);

/* GaussianBlur fused into the FAST kernel (1) or run as its own launch (0, the default; $ORBFE_FUSED).  Results
 * are identical; the fused form measured no faster and is kept as a parity-tested alternative. */
int orbfe_extractor_set_fused(orbfe_extractor *e, int enable);

/* ComputePyramid (src/ORBextractor.cc:1203-1234) and the per-level GaussianBlur (:1169-1175) as ONE kernel per level
 * -- the tile staged for the blur of level l also yields the part of level l+1 whose taps start in it -- (1, the
 * default; $ORBFE_PYRBLUR) or as separate resize and blur launches (0).  Identical results; the fused form reads every
 * level once instead of twice (KITTI +4 % stereo frames/s).  Ignored with the lane schedule and with
 * orbfe_extractor_set_fused(1). */
int orbfe_extractor_set_pyramid_blur(orbfe_extractor *e, int enable);

/* Calls of at most 8 frames (the live camera) build the pyramid with n-1 dependent resize launches of a few microseconds
 * each.  1: ONE launch instead -- a workgroup owns a tile of one level and recomputes, in LDS, the rectangles of the levels
 * below it from level 0 (k_pyramid_chain: same fixed-point step from the same inputs, identical pixels).  0 (default;
 * $ORBFE_PYR_CHAIN): the launches -- the one-launch form measured no faster (32 vs 29 us per KITTI frame). */
int orbfe_extractor_set_pyramid_chain(orbfe_extractor *e, int enable);

/* Order of the two separable passes of the 7x7 GaussianBlur kernel (src/ORBextractor.cc:1169-1175), process-wide.  Both
 * passes are exact integer sums, so the blurred bytes do not depend on it.  1 (default; $ORBFE_BLUR_HFIRST): horizontal
 * pass on the staged bytes with v_dot4_u32_u8, vertical pass on row pairs with v_dot2_u32_u16 (~160 VALU instructions per
 * wave for the two passes); 0: the rounds 1-3 form, vertical packed-16 pass first (216 per wave).  Returns the order now in force; a
 * negative argument only queries.  Takes effect at the next launch. */
int orbfe_set_blur_pass_order(int order);

/* A call's frames are split into n consecutive sub-batches that run concurrently on n HIP
 * streams with private workspace slices (1..32, default 1 or $ORBFE_STREAMS); results do not
 * depend on n.  Stage timing covers the kernels of sub-batch 0 (frames_out reports how many
 * frames those launches processed). */
int orbfe_extractor_set_streams(orbfe_extractor *e, int n);

/* Per-kernel timing, measured with HIP events on the handle's own stream (events are recorded
 * inside the calls and read back at the next synchronisation, so timing does not stall the
 * pipeline).  stage_mask: bit i enables ORBFE_STAGE_i, -1 = all, 0 = off; setting it resets the
 * accumulators.  get returns, per stage, total milliseconds and launches since the last reset. */
enum {
  ORBFE_STAGE_H2D = 0,
  ORBFE_STAGE_PYRAMID,
  ORBFE_STAGE_FAST,
  ORBFE_STAGE_OCTREE,
  ORBFE_STAGE_BLUR,
  ORBFE_STAGE_ORIENT_DESC,
  ORBFE_STAGE_D2H,
  ORBFE_STAGE_MATCH, /* batched matcher enqueued on the handle's stream (stereo / consecutive-frame BoW) */
  ORBFE_STAGE_COUNT
};
int orbfe_extractor_profile(orbfe_extractor *e, int stage_mask);
int orbfe_extractor_profile_get(orbfe_extractor *e, double *ms_out /*[ORBFE_STAGE_COUNT]*/,
                                int64_t *launches_out /*[ORBFE_STAGE_COUNT]*/,
                                double *frames_out /*[ORBFE_STAGE_COUNT], may be NULL*/);
const char *orbfe_stage_name(int stage);

/* Standalone primitives on host buffers (tests of the individual kernels). */
int orbfe_resize_linear(int device, const uint8_t *src, int sw, int sh, int sstride, uint8_t *dst,
                        int dw, int dh, int dstride);
int orbfe_gaussian_blur7_spec(int device, int spec, const uint8_t *src, int w, int h, int sstride, uint8_t *dst,
                             int dstride);
int orbfe_gaussian_blur7(int device, const uint8_t *src, int w, int h, int sstride, uint8_t *dst,
                         int dstride);

/* ------------------------------------------------------------------------- */
/* Matcher                                                                    */
/* ------------------------------------------------------------------------- */

/* DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>, ascending node id;
 * Thirdparty/DBoW2/DBoW2/FeatureVector.cpp:31-45) flattened to CSR. */
typedef struct orbfe_featvec {
  int32_t n_nodes;
  const uint32_t *node_ids; /* ascending */
  const int32_t *offsets;   /* n_nodes + 1 */
  const uint32_t *indices;  /* feature indices, grouped by node in insertion order */
} orbfe_featvec;

/* ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1828-1844) for n pairs:
 * out[i] = popcount(a[i] ^ b[i]) over 256 bits. Host buffers. */
int orbfe_descriptor_distance(int device, const uint8_t *a, const uint8_t *b, int n, int32_t *out);

/* Dense n1 x n2 Hamming matrix (row-major int16 would do; int32 for simplicity). Host buffers. */
int orbfe_hamming_matrix(int device, const uint8_t *desc1, int n1, const uint8_t *desc2, int n2,
                         int32_t *out);

/* ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>&)  (src/ORBmatcher.cc:185-325).
 * has_mp1[i] != 0 <=> KF feature i has a non-bad MapPoint.  match_f[j] (size n2) = index of the KF
 * feature whose MapPoint the wrapper assigns to frame feature j, or -1.  Returns nmatches >= 0,
 * or a negative status. */
int orbfe_search_by_bow(int device, const uint8_t *desc1, const uint8_t *has_mp1,
                        const float *angle1, int n1, const orbfe_featvec *fv1,
                        const uint8_t *desc2, const float *angle2, int n2,
                        const orbfe_featvec *fv2, float nnratio, int check_orientation,
                        int32_t *match_f);

/* ORBmatcher::SearchByBoW(KeyFrame*, KeyFrame*, vector<MapPoint*>&)  (src/ORBmatcher.cc:610-743).
 * match12[i] (size n1) = KF2 feature index or -1. */
int orbfe_search_by_bow_kf(int device, const uint8_t *desc1, const uint8_t *has_mp1,
                           const float *angle1, int n1, const orbfe_featvec *fv1,
                           const uint8_t *desc2, const uint8_t *has_mp2, const float *angle2,
                           int n2, const orbfe_featvec *fv2, float nnratio, int check_orientation,
                           int32_t *match12);

/* ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, cv::Mat F12,
 * vector<pair<size_t,size_t>>&, bool bOnlyStereo)  (src/ORBmatcher.cc:754-928).
 * Keypoints are mvKeysUn as SoA; stereo flags are (mvuRight[i] >= 0); F12 is row-major 3x3;
 * (ex,ey) the epipole computed by the caller as at :766-769; scale_factors2 / level_sigma2_2 are
 * KF2's mvScaleFactors / mvLevelSigma2.  match12[i] = KF2 index or -1; the wrapper emits the
 * pairs in ascending i exactly as :920-925. */
int orbfe_search_for_triangulation(int device, const uint8_t *desc1, const uint8_t *has_mp1,
                                   const float *x1, const float *y1, const float *angle1,
                                   const uint8_t *stereo1, int n1, const orbfe_featvec *fv1,
                                   const uint8_t *desc2, const uint8_t *has_mp2, const float *x2,
                                   const float *y2, const float *angle2, const int32_t *octave2,
                                   const uint8_t *stereo2, int n2, const orbfe_featvec *fv2,
                                   const float *F12, float ex, float ey,
                                   const float *scale_factors2, const float *level_sigma2_2,
                                   int n_levels2, int only_stereo, int check_orientation,
                                   int32_t *match12);

/* Frame::ComputeStereoMatches()  (src/Frame.cc:512-686).  `left`/`right` are the two extractor
 * handles whose LAST extract call produced the keypoints (their pyramids are read on the device,
 * replacing mpORBextractorLeft/Right->mvImagePyramid); frameL/frameR select the frame of that
 * batch.  kp/desc are host arrays exactly as returned by orbfe_extract.  Outputs mvuRight / mvDepth
 * (N floats each, -1 = no stereo).  mbf, mb as in src/Frame.cc:114,542-544. */
int orbfe_compute_stereo_matches(orbfe_extractor *left, int frameL, orbfe_extractor *right,
                                 int frameR, const orbfe_keypoint *kpL, const uint8_t *descL,
                                 int N, const orbfe_keypoint *kpR, const uint8_t *descR, int Nr,
                                 float mbf, float mb, float *uRight, float *depth);

/* The same for a device-resident batch: the handle's LAST orbfe_extract_batch_device(_async) call
 * processed frames L0,R0,L1,R1,... (pair p = frames 2p, 2p+1, both images through ONE handle);
 * d_keypoints / d_descriptors / d_n are that call's outputs (same capacity).  Writes mvuRight and
 * mvDepth of pair p at [p*capacity + i] (i < capacity; -1 beyond the left frame's keypoints) and
 * the number of surviving stereo matches at d_n_stereo[p].  Enqueued on the handle's stream after
 * the extraction; wait with orbfe_extractor_synchronize. */
int orbfe_stereo_match_batch_device(orbfe_extractor *e, int n_pairs, const orbfe_keypoint *d_keypoints,
                                    const uint8_t *d_descriptors, const int32_t *d_n, int capacity,
                                    float mbf, float mb, float *d_uRight, float *d_depth,
                                    int32_t *d_n_stereo);

/* The front end of the stereo Frame constructor in ONE call (src/Frame.cc:78-96: ExtractORB(0, imLeft) and
 * ExtractORB(1, imRight) on two threads, join, ComputeStereoMatches): both eyes go through handle e as a two-frame
 * batch, the stereo matcher runs on the records while they are still in HBM, and keypoints / descriptors of both eyes,
 * mvuRight and mvDepth (n_left floats each, -1 = no stereo) come back in one download.  Same results as two
 * orbfe_extract calls + orbfe_compute_stereo_matches.  The handle then holds the pair as frames 0 (left) and 1 (right):
 * orbfe_frame_from_extractor(e, 0, ...) builds the resident Frame from it. */
int orbfe_extract_stereo_frame(orbfe_extractor *e, const uint8_t *left, const uint8_t *right, int width, int height,
                               int stride, orbfe_keypoint *kp_left, uint8_t *desc_left, int *n_left,
                               orbfe_keypoint *kp_right, uint8_t *desc_right, int *n_right, int capacity, float mbf,
                               float mb, float *uRight, float *depth);

/* ------------------------------------------------------------------------- */
/* DBoW2 vocabulary (the step right before SearchByBoW)       */
/* ------------------------------------------------------------------------- */
typedef struct orbfe_vocabulary orbfe_vocabulary;

/* TemplatedVocabulary::loadFromTextFile (Thirdparty/DBoW2/DBoW2/TemplatedVocabulary.h:1338-1424):
 * first line "k L scoring weighting", then one node per line "parent is_leaf d0..d31 weight".
 * Deviation: empty lines are ignored (the reference turns the file's trailing empty line into a
 * child of the root with an UNINITIALISED descriptor). */
int orbfe_vocabulary_load_text(const char *path, int device, orbfe_vocabulary **out);
/* The same tree from arrays -- what the node lines of the text file hold (:1374-1417): entry i is node i+1 (the
 * root is node 0), parent[i] the NodeId of its parent, is_leaf[i] != 0 makes it the next word (word ids count leaves
 * in array order, :1402-1408), descriptors[32*i ..] and weight[i] as in the line.  k, L, scoring, weighting = the
 * header line.  For callers that hold or convert a vocabulary in memory (ORBvoc.txt is 145 MB of text). */
int orbfe_vocabulary_create(int k, int L, int scoring, int weighting, int n_nodes, const int32_t *parent,
                            const uint8_t *is_leaf, const uint8_t *descriptors, const double *weight,
                            int device, orbfe_vocabulary **out);
void orbfe_vocabulary_destroy(orbfe_vocabulary *v);
int orbfe_vocabulary_info(const orbfe_vocabulary *v, int *k, int *L, int *n_nodes, int *n_words);

/* transform(feature, word_id, weight, nid, levelsup) (:1218-1259) for n host descriptors: the
 * k-ary descent with FORB::distance.  Features with weight > 0 are the ones transform(features,
 * BowVector&, FeatureVector&, levelsup) (:1127-1194; called with levelsup = 4 at src/Frame.cc:438)
 * adds as BowVector.addWeight(word_id, weight) / FeatureVector.addFeature(node_id, i).  Returns
 * their number, or a negative status.  Runs on the calling thread's matcher stream and is complete on
 * return; the tree is immutable after create and the call keeps nothing on the handle, so several
 * threads may make it on one handle at once (Frame::ComputeBoW on tracking, KeyFrame::ComputeBoW on
 * local mapping). */
int orbfe_vocabulary_transform(orbfe_vocabulary *v, const uint8_t *descriptors, int n, int levelsup,
                               uint32_t *word_id, double *weight, uint32_t *node_id);

/* Frame::ComputeBoW for every frame of a device-resident extractor batch: FeatureVector f as CSR at
 * d_fv_nodes[f*capacity ..] (ascending, d_fv_count[f] of them), d_fv_offsets[f*(capacity+1) ..],
 * d_fv_indices[f*capacity ..]; optional per-feature word ids / weights (both or neither).  Runs on the
 * calling thread's matcher stream -- the caller's writes of the inputs must have completed -- and is
 * complete on return; may be made on one handle from several threads at once, like the call above. */
int orbfe_vocabulary_featvec_batch_device(orbfe_vocabulary *v, const uint8_t *d_descriptors,
                                          const int32_t *d_n, int n_frames, int capacity, int levelsup,
                                          uint32_t *d_fv_nodes, int32_t *d_fv_offsets,
                                          uint32_t *d_fv_indices, int32_t *d_fv_count, uint32_t *d_word,
                                          double *d_weight);

/* ComputeBoW + SearchByBoW(KF = frame t-1, F = frame t) for t = 1..n_frames-1 of a device-resident
 * batch (every KF feature counts as having a MapPoint): d_match[(t-1)*capacity + j] = index of the
 * frame t-1 feature matched to feature j of frame t, or -1; d_nmatches[t-1] = nmatches. */
int orbfe_bow_match_consecutive_batch_device(orbfe_vocabulary *v, int n_frames,
                                             const orbfe_keypoint *d_keypoints,
                                             const uint8_t *d_descriptors, const int32_t *d_n,
                                             int capacity, int levelsup, float nnratio,
                                             int check_orientation, int32_t *d_match,
                                             int32_t *d_nmatches);
/* The same, enqueued on extractor e's stream behind every sub-batch of its last
 * orbfe_extract_batch_device_async call (ordered on the device, no host wait); returns at once,
 * orbfe_extractor_synchronize(e) waits.  The next extract call on e may be enqueued right away: its
 * sub-batch streams wait for this matcher before they overwrite the keypoints it reads. */
int orbfe_bow_match_consecutive_batch_device_async(orbfe_vocabulary *v, orbfe_extractor *e, int n_frames,
                                                   const orbfe_keypoint *d_keypoints,
                                                   const uint8_t *d_descriptors, const int32_t *d_n,
                                                   int capacity, int levelsup, float nnratio,
                                                   int check_orientation, int32_t *d_match,
                                                   int32_t *d_nmatches);

/* The same over the LEFT frames of an (L0, R0, L1, R1, ...) stereo batch of extractor e -- a stereo Frame's
 * ComputeBoW / SearchByBoW use its left keypoints (mvKeys, mDescriptors; src/Frame.cc:61-117): pair t-1 against
 * pair t for t = 1..n_pairs-1; d_match[(t-1)*capacity + j], d_nmatches[t-1] as above.  d_keypoints / d_descriptors /
 * d_n are the extractor batch's arrays (2*n_pairs frames). */
int orbfe_bow_match_consecutive_stereo_batch_device_async(orbfe_vocabulary *v, orbfe_extractor *e, int n_pairs,
                                                          const orbfe_keypoint *d_keypoints,
                                                          const uint8_t *d_descriptors, const int32_t *d_n,
                                                          int capacity, int levelsup, float nnratio,
                                                          int check_orientation, int32_t *d_match,
                                                          int32_t *d_nmatches);

/* The BowVector of transform(features, BowVector&, FeatureVector&, levelsup) (:1127-1194): addWeight in
 * feature order for the features with weight > 0, then the L1 normalisation (sum of fabs in ascending word
 * order, one division per entry; Thirdparty/DBoW2/DBoW2/BowVector.cpp:34-84).  word_ids ascend and are
 * unique, *n_words of them; more than `capacity` returns ORBFE_ERR_CAPACITY with *n_words set.  Only
 * L1_NORM / TF_IDF vocabularies (header "k L 0 0", what ORBvoc.txt is): others return ORBFE_ERR_INVALID. */
int orbfe_vocabulary_transform_bow(orbfe_vocabulary *v, const uint8_t *descriptors, int n, int levelsup,
                                   uint32_t *word_ids, double *values, int capacity, int *n_words);

/* ------------------------------------------------------------------------- */
/* KeyFrameDatabase (src/KeyFrameDatabase.cc): BoW scores, loop / reloc sets  */
/* ------------------------------------------------------------------------- */
/* The BowVectors of the key frames, resident on the device, in the order of the reference's per-word lists
 * (insertion order).  A handle serialises its own calls; creating one does not touch the device (the first
 * call that uploads does), every later call needs it. */
typedef struct orbfe_kfdb orbfe_kfdb;
enum { ORBFE_KFDB_RELOC = 0, ORBFE_KFDB_LOOP = 1 };

/* n_words: the vocabulary's word count (mvInvertedFile.resize(voc.size()), :36). */
int orbfe_kfdb_create(int n_words, int device, orbfe_kfdb **out);
void orbfe_kfdb_destroy(orbfe_kfdb *db);
/* KeyFrameDatabase::add (:43-49) with pKF->mBowVec as n ascending unique word ids + values, checked on the
 * host before anything is uploaded: ids that do not ascend strictly or reach n_words return ORBFE_ERR_INVALID.
 * Deviation: an id already in the database returns ORBFE_ERR_INVALID (the reference would list it twice). */
int orbfe_kfdb_add(orbfe_kfdb *db, int64_t kf_id, const uint32_t *word_ids, const double *values, int n);
/* KeyFrameDatabase::erase (:51-70): the others keep their relative order, and a later add of the same id goes
 * to the end.  Returns 1, or 0 when the id is not in the database; a negative status means nothing was erased. */
int orbfe_kfdb_erase(orbfe_kfdb *db, int64_t kf_id);
int orbfe_kfdb_clear(orbfe_kfdb *db);
int orbfe_kfdb_size(const orbfe_kfdb *db);

/* The scored set of DetectLoopCandidates (:106-160) / DetectRelocalizationCandidates (:236-288) for n_queries
 * BowVectors in one call: query q is q_words / q_values [q_offsets[q], q_offsets[q+1]) (ascending unique ids),
 * and the key frames excl_ids [excl_offsets[q], excl_offsets[q+1]) -- pKF->GetConnectedKeyFrames() of the loop
 * form; excl_offsets NULL = none, ids the database does not hold are ignored -- take no part in it.  Per query:
 * the key frames sharing more than (int)(maxCommonWords * 0.8f) words, in the order of the reference's
 * lKFsSharingWords, as kf_id / n_common (mnLoopWords, mnRelocWords) / score ((float) of L1Scoring::score,
 * Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68, query first) [q * capacity ..], count[q] of them.  A count
 * above `capacity` fills `capacity` entries and returns ORBFE_ERR_CAPACITY (every count[] is still set).  At most
 * 65535 queries per call (more returns ORBFE_ERR_INVALID). */
int orbfe_kfdb_query(orbfe_kfdb *db, int n_queries, const int32_t *q_offsets, const uint32_t *q_words,
                     const double *q_values, const int32_t *excl_offsets, const int64_t *excl_ids, int capacity,
                     int64_t *kf_id, int32_t *n_common, float *score, int32_t *count);
/* mpVoc->score(query, pKF->mBowVec) in double for n_ids named key frames (LoopClosing::DetectLoop's minScore,
 * src/LoopClosing.cc:143-158); an id the database does not hold returns ORBFE_ERR_INVALID. */
int orbfe_kfdb_score(orbfe_kfdb *db, const uint32_t *q_words, const double *q_values, int n, int n_ids,
                     const int64_t *kf_ids, double *scores);
/* The covisibility stage of both functions (:165-218 mode ORBFE_KFDB_LOOP, :293-346 ORBFE_KFDB_RELOC; min_score
 * is read in loop mode only) over ONE query's scored set: entry i's GetBestCovisibilityKeyFrames(10) is
 * neigh_ids [neigh_offsets[i], neigh_offsets[i+1]) in the caller's order.  Returns the candidate ids in group
 * order, *n_out of them (ORBFE_ERR_CAPACITY when more than `capacity`).  Host code: needs no device. */
int orbfe_kfdb_group_candidates(int mode, float min_score, int n, const int64_t *kf_id, const int32_t *n_common,
                                const float *score, const int32_t *neigh_offsets, const int64_t *neigh_ids,
                                int64_t *out_ids, int capacity, int *n_out);

/* ------------------------------------------------------------------------- */
/* Next to the path                                */
/* ------------------------------------------------------------------------- */

/* cv::cvtColor(im, im, CV_RGB2GRAY | CV_BGR2GRAY | CV_RGBA2GRAY | CV_BGRA2GRAY) of
 * Tracking::GrabImage{Stereo,RGBD,Monocular} (src/Tracking.cc:176-262), 8-bit, channels 3 or 4,
 * rgb_order != 0 for RGB(A) input: (R*4899 + G*9617 + B*1868 + 2^13) >> 14.  Host buffers: `width`
 * pixels of each row are read / written, the padding up to the stride is left alone.  This and the other
 * host-array calls of this section and of the rectifier / undistortion section below (orbfe_distinctive_
 * descriptors, orbfe_rectifier_create, orbfe_remap, orbfe_init_undistort_rectify_map, orbfe_undistort_points,
 * orbfe_compute_image_bounds, orbfe_stereo_from_rgbd) run on the calling thread's matcher stream and are
 * complete on return. */
int orbfe_cvt_gray(int device, const uint8_t *src, int width, int height, int stride, int channels,
                   int rgb_order, uint8_t *dst, int dst_stride);
/* Same on device-resident frames (so colour input never round-trips through the host).  This and the
 * other two device-pointer calls of these sections (orbfe_remap_batch_device, orbfe_undistort_keypoints_
 * batch_device) are enqueued on the default stream, complete on return: the library knows no stream for
 * arrays the caller wrote, and the default stream orders the kernel behind the caller's default-stream
 * work.  The call waits for that stream alone, not for the device. */
int orbfe_cvt_gray_batch_device(int device, const uint8_t *d_src, int n_frames, int width, int height,
                                int stride, size_t frame_stride, int channels, int rgb_order,
                                uint8_t *d_dst, int dst_stride, size_t dst_frame_stride);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) for n_points map points at once:
 * map point m owns descriptors [offsets[m], offsets[m+1]) (its observations, 32 bytes each);
 * best_index[m] = index inside that range of the descriptor with the least median Hamming distance
 * to the others (median = sorted row [(size_t)(0.5*(n-1))]; first minimum wins), -1 if empty. */
int orbfe_distinctive_descriptors(int device, const uint8_t *descriptors, const int32_t *offsets,
                                  int n_points, int32_t *best_index);

/* ------------------------------------------------------------------------- */
/* Tracking-thread projection searches                */
/* ------------------------------------------------------------------------- */

/* The fields of an ORB_SLAM2::Frame the searches read (include/Frame.h:120-190): the undistorted
 * keypoints mvKeysUn split into arrays, mvuRight, mDescriptors and the undistorted image bounds
 * mnMinX..mnMaxY (src/Frame.cc:697-728).  At most 16384 keypoints. */
typedef struct orbfe_frame_view {
  int32_t n;
  const float *x, *y;       /* mvKeysUn[i].pt */
  const int32_t *octave;    /* mvKeysUn[i].octave */
  const float *angle;       /* mvKeysUn[i].angle (only read with check_orientation) */
  const float *u_right;     /* mvuRight, NULL for monocular frames */
  const uint8_t *desc;      /* mDescriptors, n x 32 */
  float min_x, max_x, min_y, max_y;
  const struct orbfe_frame *resident; /* NULL, or the handle orbfe_frame_upload made of this frame: the search then
                                         uploads nothing of the frame (use orbfe_frame_get_view) */
} orbfe_frame_view;

/* Device-resident Frame / KeyFrame operands.  LocalMapping matches one key frame against 10-20 neighbours
 * (src/LocalMapping.cc:256-315, 517-573), relocalisation one frame against several candidates
 * (src/Tracking.cc:1478-1498): orbfe_frame_upload moves what a frame contributes to any search -- keypoint arrays,
 * descriptors, the 64 x 48 grid of Frame::AssignFeaturesToGrid (built once), the FeatureVector's index list (fv may be
 * NULL for frames that only take part in projection searches) -- to the device once.  The view needs x, y, octave,
 * desc and the bounds; angle / u_right as the searches it will take part in need them.  The handle copies what it
 * needs (the caller's arrays may go away), is immutable, and may be used from any thread concurrently. */
typedef struct orbfe_frame orbfe_frame;
int orbfe_frame_upload(int device, const orbfe_frame_view *view, const orbfe_featvec *fv, orbfe_frame **out);
void orbfe_frame_release(orbfe_frame *f);
/* The handle's own view (host copies inside the handle, `resident` set): pass it wherever an orbfe_frame_view is
 * taken.  Valid until orbfe_frame_release. */
const orbfe_frame_view *orbfe_frame_get_view(const orbfe_frame *f);

/* Frame::Frame (src/Frame.cc:61-117) is ExtractORB -> UndistortKeyPoints -> ComputeStereoMatches -> AssignFeaturesToGrid:
 * when the Frame is built the extractor's keypoint records and descriptors are still in HBM.  These two build the
 * resident operands FROM THEM -- records split into the x / y / angle / octave arrays, descriptors copied device to device,
 * grid built on the device -- so of a frame's 60 bytes per keypoint only mvuRight (and, with ORBFE_FRAME_XY_FROM_VIEW, the
 * caller's undistorted positions) cross PCIe.  `view` holds the host arrays the argument checks and the host-pointer forms read
 * (mvKeysUn / mvuRight / mDescriptors as the caller has them after its own constructor steps); view->n records are taken.
 *   orbfe_frame_from_extractor: frame `frame` of the handle's last orbfe_extract / small orbfe_extract_batch call
 *       (ORBFE_ERR_INVALID after a device-batch or pipelined call: those outputs are the caller's);
 *       The handle's next call that rewrites its output block waits (on the device) for the build to finish reading it;
 *   orbfe_frame_from_device:    any device arrays in the extractor's output layout (orbfe_extract_batch_device outputs at
 *       d_keypoints + frame * capacity, d_descriptors + frame * capacity * 32), complete when the call is made.  The
 *       build reads them on the calling thread's stream after the call has returned: they must stay unmodified and
 *       allocated until orbfe_frame_synchronize(*out) has returned (or a search on the frame has returned).
 * Like orbfe_frame_upload neither waits for the device: searches are ordered behind the build by the frame's own event.
 * Released slabs are pooled (no hipMalloc / hipFree -- which waits for the whole device -- per key frame). */
#define ORBFE_FRAME_XY_FROM_VIEW 1 /* x / y come from `view` (undistorted by the caller: cameras with distortion) */
int orbfe_frame_from_extractor(orbfe_extractor *e, int frame, const orbfe_frame_view *view, const orbfe_featvec *fv,
                               int flags, orbfe_frame **out);
int orbfe_frame_from_device(int device, const orbfe_keypoint *d_keypoints, const uint8_t *d_descriptors,
                            const orbfe_frame_view *view, const orbfe_featvec *fv, int flags, orbfe_frame **out);
/* Frame::ComputeBoW runs after the constructor (src/Tracking.cc:836-843, src/Frame.cc:433-440): attach the FeatureVector
 * to a frame made resident without one.  Call it before any search uses the frame (it rewrites the frame's index list);
 * the calling thread may differ from the one that built the frame: the index copy is ordered behind the frame's build,
 * and the call returns once both have completed. */
int orbfe_frame_set_featvec(orbfe_frame *f, const orbfe_featvec *fv);
/* Returns once the frame's build (upload / copy from device records + grid build) has completed on the device: after it,
 * the device arrays given to orbfe_frame_from_device may be reused. */
int orbfe_frame_synchronize(const orbfe_frame *f);

/* Test hooks (tests/stream_order.py), never used by a product path.  A one-wave kernel that holds a stream for `usec`
 * microseconds (0 .. 1 000 000; 0 = a marker that completes at once) and writes no memory; the call returns without
 * waiting.  `stream` of an extractor: 0 = its stream 0, 1 .. 31 = sub-batch stream 1 .. 31 (the lane schedule: P = 1,
 * V = 2, T = 0), ORBFE_DEBUG_STREAM_H2D / _D2H = the copy streams of the pipelined host path; a stream the handle has not
 * created yet is ORBFE_ERR_INVALID.  The thread form holds the calling thread's matcher stream on `device` (created if
 * needed).  The _idle queries return 1 when everything enqueued on the stream has completed, 0 while work is pending. */
#define ORBFE_DEBUG_STREAM_H2D (-1)
#define ORBFE_DEBUG_STREAM_D2H (-2)
int orbfe_debug_stall_extractor_stream(orbfe_extractor *e, int stream, int usec);
int orbfe_debug_extractor_stream_idle(orbfe_extractor *e, int stream);
int orbfe_debug_stall_thread_stream(int device, int usec);
int orbfe_debug_thread_stream_idle(int device);

/* Frame::AssignFeaturesToGrid + Frame::GetFeaturesInArea (src/Frame.cc:246-267, 358-427) for
 * n_queries windows at once: count[q] features lie in the window of query q; the first
 * min(count[q], capacity) of them -- in the reference's order (grid column, grid row, feature
 * index) -- are written to indices[q*capacity ..].  ORBFE_ERR_CAPACITY (counts still exact) when a
 * window holds more than `capacity` features. */
int orbfe_features_in_area(int device, const orbfe_frame_view *frame, int n_queries, const float *x,
                           const float *y, const float *r, const int32_t *min_level,
                           const int32_t *max_level, int capacity, int32_t *count, int32_t *indices);

/* ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th)
 * (src/ORBmatcher.cc:51-138).  Map point i is described by what Frame::isInFrustum left on it:
 * in_view (mbTrackInView && !isBad()), level (mnTrackScaleLevel), view_cos (mTrackViewCos), proj_x /
 * proj_y / proj_xr (mTrackProjX/Y/XR), mp_desc (GetDescriptor()), mp_obs_positive (Observations()>0,
 * NULL = all).  blocked[idx] != 0 <=> F.mvpMapPoints[idx] already holds a point with observations
 * (NULL = none).  match[idx] = map point assigned to frame feature idx or -1; *n_matches as the
 * reference counts them. */
int orbfe_search_by_projection(int device, const orbfe_frame_view *F, const float *scale_factors,
                               int n_levels, const uint8_t *blocked, int n_mp, const uint8_t *in_view,
                               const int32_t *level, const float *view_cos, const float *proj_x,
                               const float *proj_y, const float *proj_xr, const uint8_t *mp_desc,
                               const uint8_t *mp_obs_positive, float th, float nnratio,
                               int32_t *match, int32_t *n_matches);

/* ------------------------------------------------------------------------- */
/* Device-resident map points: Frame::isInFrustum + Tracking::SearchLocalPoints */
/* ------------------------------------------------------------------------- */
/* What isInFrustum and SearchByProjection read of a MapPoint (mWorldPos, mNormalVector, mfMinDistance, mfMaxDistance,
 * mDescriptor, isBad(), Observations() > 0), resident on the device and indexed by SLOT: the caller keeps the
 * MapPoint* <-> slot map, as it keeps the ids of the key-frame database.  The local map hardly changes between
 * consecutive frames, so per frame only a slot list, the masks and the pose travel.  Creating a table does not touch
 * the device (the first update or use does); a slot that was never updated counts as bad.  A handle serialises its own
 * calls. */
typedef struct orbfe_mappoints orbfe_mappoints;
#define ORBFE_MP_BAD 1          /* flags bit 0: MapPoint::isBad() */
#define ORBFE_MP_OBSERVED 2     /* flags bit 1: MapPoint::Observations() > 0 */
int orbfe_mappoints_create(int device, int capacity, orbfe_mappoints **out);
void orbfe_mappoints_destroy(orbfe_mappoints *mp);
int orbfe_mappoints_capacity(const orbfe_mappoints *mp);
/* Writes n slots: pos = GetWorldPos(), normal = GetNormal() (3 floats each), min_dist / max_dist the RAW mfMinDistance /
 * mfMaxDistance (the 0.8f / 1.2f of GetMinDistanceInvariance / GetMaxDistanceInvariance, src/MapPoint.cc, are applied
 * on the device), desc = GetDescriptor() (32 bytes each; NULL keeps the descriptors the slots hold), flags as above.
 * Slots outside [0, capacity), n < 0 and NULL arrays return ORBFE_ERR_INVALID before anything is enqueued; a slot named
 * twice in one call takes either entry.  Enqueued on the calling thread's matcher stream and complete on return, so
 * the table may be used from any thread afterwards. */
int orbfe_mappoints_update(orbfe_mappoints *mp, int n, const int32_t *slot, const float *pos, const float *normal,
                           const float *min_dist, const float *max_dist, const uint8_t *desc, const uint8_t *flags);

/* The fields of the Frame isInFrustum reads (src/Frame.cc:292-353): mRcw (row-major), mtcw, mOw, fx, fy, cx, cy, mbf,
 * mnMinX .. mnMaxY, mfLogScaleFactor, mnScaleLevels. */
typedef struct orbfe_camera_pose {
  float Rcw[9], tcw[3], Ow[3];
  float fx, fy, cx, cy, mbf;
  float min_x, max_x, min_y, max_y;
  float log_scale_factor;
  int32_t n_levels;
} orbfe_camera_pose;

/* Frame::isInFrustum(pMP, viewingCosLimit) (src/Frame.cc:292-353) with MapPoint::PredictScale for the n map points in
 * slot[]; skip[i] != 0 (NULL = none) leaves point i out, as the points already matched in the frame are
 * (mnLastFrameSeen, src/Tracking.cc SearchLocalPoints).  in_view[i] = !skip && !bad && every test passes; where it is
 * set, level / view_cos / proj_x / proj_y / proj_xr are mnTrackScaleLevel / mTrackViewCos / mTrackProjX / Y / XR and
 * inv_z / dist the 1/z and the distance to the camera centre behind them; elsewhere they are 0.  IEEE binary32, no
 * contraction, sums left to right:
 *   xc = ((R00*X + R01*Y) + R02*Z) + t0 (yc, zc likewise); reject zc < 0; invz = 1/zc; u = (fx*xc)*invz + cx;
 *   v = (fy*yc)*invz + cy; reject u < min_x || u > max_x || v < min_y || v > max_y; PO = P - Ow;
 *   dist = (float)sqrt(sum (double)PO_i^2); reject dist < 0.8f*min || dist > 1.2f*max;
 *   view_cos = (float)(sum (double)PO_i*(double)Pn_i / (double)dist); reject view_cos < limit;
 *   level = clamp(ceil(log((double)(max/dist)) / (double)log_scale_factor), 0, n_levels-1); proj_xr = u - mbf*invz.
 * Only the slot list, the mask and the pose go up.  Any output may be NULL. */
int orbfe_project_in_frustum(orbfe_mappoints *mp, int n, const int32_t *slot, const uint8_t *skip,
                             const orbfe_camera_pose *pose, float viewing_cos_limit, uint8_t *in_view, int32_t *level,
                             float *view_cos, float *proj_x, float *proj_y, float *proj_xr, float *inv_z, float *dist);

/* Tracking::SearchLocalPoints (src/Tracking.cc) as ONE call: the projection above writes the query windows of
 * orbfe_search_by_projection (RadiusByViewingCos(view_cos) * th * scale_factors[level], levels [level-1, level], the
 * points' descriptors gathered from the table) directly in device memory, and the window search and the claim loop run
 * behind it on the same stream.  match[idx] = position in slot[] of the point assigned to frame feature idx, or -1;
 * *n_matches as the reference counts them; in_view (optional, n bytes) for IncreaseVisible.  Equal to
 * orbfe_search_by_projection fed with orbfe_project_in_frustum's outputs, the table's descriptors and
 * mp_obs_positive = flags bit 1.  pose->n_levels must not exceed n_levels. */
int orbfe_search_local_points(orbfe_mappoints *mp, int n, const int32_t *slot, const uint8_t *skip,
                              const orbfe_camera_pose *pose, float viewing_cos_limit, const orbfe_frame_view *F,
                              const float *scale_factors, int n_levels, const uint8_t *blocked, float th, float nnratio,
                              int32_t *match, int32_t *n_matches, uint8_t *in_view);

/* The prologue of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1516-1550), the search
 * Tracking::TrackWithMotionModel runs on every frame, for a COMPACT list: slot[i] / last_octave[i] / skip[i] name only the
 * last-frame features that hold a non-outlier map point (:1510-1514), in ascending feature order -- the claim loop depends on
 * that order.  pose = the current frame's (motion-model) pose.  Outputs hold n entries; any may be NULL.  valid[i] = the point
 * passes every test; where it is set, u / v / inv_z / ur / radius are the projection, 1/zc, u - mbf/zc and the window radius;
 * elsewhere they are 0.  IEEE binary32, no contraction, sums left to right, in this order:
 *   reject skip[i] (NULL = none); flags & ORBFE_MP_BAD is NOT tested -- the reference asks pMP and mvbOutlier[i] only;
 *   xc = ((R00*X + R01*Y) + R02*Z) + t0 (yc, zc likewise); invz = 1/zc (the reference's 1.0/z in double, rounded to float, is
 *   the same float quotient: 53 >= 2*24 + 2); reject invz < 0; u = (fx*xc)*invz + cx; v = (fy*yc)*invz + cy;
 *   keep only u >= min_x && u <= max_x && v >= min_y && v <= max_y -- the bounds are inclusive.  This differs from the
 *   reference's four rejects (u < min_x || u > max_x, v likewise) only for a NaN coordinate (zc == 0 with xc == 0), which is
 *   rejected here; the reference would pass it on to GetFeaturesInArea, whose float-to-int conversions are then undefined;
 *   ur = u - mbf*invz; radius = th * scale_factors[last_octave].
 * mode selects the levels searched, as for orbfe_search_by_projection_last_frame: 0 [octave-1, octave+1], 1 (bForward)
 * >= octave, 2 (bBackward) <= octave; the caller computes it from tlc (:1497-1506).  Only the slot list, the mask, the
 * octaves, the pose and the level table go up.  A slot outside the table (-1 included), an octave outside [0, n_levels),
 * pose->n_levels outside 1 .. min(64, n_levels), n < 0, a mode other than 0 / 1 / 2 and NULL slot / last_octave / pose /
 * scale_factors return ORBFE_ERR_INVALID before anything is enqueued; n == 0 is ORBFE_OK with nothing touched. */
int orbfe_project_last_frame(orbfe_mappoints *mp, int n, const int32_t *slot, const uint8_t *skip /* [n] or NULL */,
                             const int32_t *last_octave, const orbfe_camera_pose *pose, const float *scale_factors, int n_levels,
                             float th, int mode, uint8_t *valid, float *u, float *v, float *inv_z, float *ur, float *radius);

/* SearchByProjection(CurrentFrame, LastFrame, th, bMono) (src/ORBmatcher.cc:1484-1633) as ONE call: the projection above
 * writes the query windows of orbfe_search_by_projection_last_frame (centre (u, v), radius, the level range of `mode`, ur for
 * the stereo check of :1567-1573 when Cur has u_right), gathers the points' descriptors from the table and takes
 * obs_positive from flags bit ORBFE_MP_OBSERVED; the window search and the claim loop (TH_HIGH, the rotation histogram with
 * last_angle[i] = LastFrame.mvKeysUn[.].angle) run behind it on the same stream.  One upload (slot list, mask, octaves,
 * angles, pose, level table, blocked), one download.  match_cur[i2] = POSITION IN slot[] of the point given to feature i2 of
 * Cur, or -1 -- what orbfe_pose_optimization_mappoints takes with the same slot[], so the two chain without repacking;
 * *n_matches as the reference counts them; valid_out (optional, n bytes) = the points that were searched.  Cur may be a
 * host view or a resident frame.  blocked as for orbfe_search_by_projection_last_frame (NULL = none).  Equal to
 * orbfe_search_by_projection_last_frame fed with orbfe_project_last_frame's outputs, the table's descriptors and
 * obs_positive = flags bit 1, bit for bit.  Beyond orbfe_project_last_frame's checks: a bad Cur, NULL match_cur / n_matches
 * and -- with check_orientation -- NULL angles return ORBFE_ERR_INVALID before anything is enqueued.
 * What stays with the caller: mode from tlc, the retry with 2*th when fewer than 20 matches come back
 * (src/Tracking.cc:969-973), and everything behind the pose optimisation (:985-1010). */
int orbfe_search_last_frame_mappoints(orbfe_mappoints *mp, int n, const int32_t *slot, const uint8_t *skip,
                                      const int32_t *last_octave, const float *last_angle, const orbfe_camera_pose *pose,
                                      const orbfe_frame_view *Cur, const float *scale_factors, int n_levels,
                                      const uint8_t *blocked, int mode, float th, int check_orientation, int32_t *match_cur,
                                      int32_t *n_matches, uint8_t *valid_out /* [n] or NULL */);

/* The prologue of ORBmatcher::SearchByProjection(CurrentFrame, pKF, sAlreadyFound, th, ORBdist) (src/ORBmatcher.cc:1665-1699,
 * Tracking::Relocalization) for n_candidates (<= 64) jobs in ONE kernel launch.  Job k owns entries [offsets[k],
 * offsets[k+1]) of the concatenated slot[] / skip[] -- pKF_k's non-null map points in feature order, skip = sAlreadyFound --
 * and pose[k], the current frame's pose for that candidate.  offsets[0] = 0; offsets never descend; a job may be empty.
 * Outputs hold offsets[n_candidates] entries; any may be NULL; where valid is 0 the others are 0.  In this order:
 *   reject flags & ORBFE_MP_BAD; reject skip[i] (NULL = none); xc, yc, zc, invz, u, v and the inclusive image test as for
 *   orbfe_project_last_frame -- there is NO depth-sign test, the reference has none; PO = P - Ow;
 *   dist = (float)sqrt(sum (double)PO_i^2); reject dist < 0.8f*min || dist > 1.2f*max; no viewing-angle test;
 *   level = clamp(ceil(log((double)(max/dist)) / (double)log_scale_factor), 0, n_levels-1) (MapPoint::PredictScale).
 * A slot outside the table, n_candidates outside 0 .. 64, offsets that do not start at 0 or descend, a pose whose n_levels is
 * not 1 .. 64 and NULL offsets / slot / pose return ORBFE_ERR_INVALID before anything is enqueued; n_candidates == 0 or no
 * point at all is ORBFE_OK with nothing touched. */
int orbfe_project_keyframe(orbfe_mappoints *mp, int n_candidates, const int32_t *offsets /* [n_candidates + 1] */,
                           const int32_t *slot, const uint8_t *skip, const orbfe_camera_pose *pose /* [n_candidates] */,
                           uint8_t *valid, float *u, float *v, float *inv_z, int32_t *level, float *dist);

/* The relocalisation search for K candidates as ONE call: the projection above writes the windows of
 * orbfe_search_by_projection_keyframe_multi (radius th[k] * scale_factors[level], levels [level-1, level+1]) and gathers the
 * descriptors; the K window searches and claim loops (bound orb_dist[k], blocked[k] = Cur.mvpMapPoints[i2] != NULL at entry,
 * blocked or blocked[k] may be NULL, kf_angle[i] = pKF_k->mvKeysUn[.].angle over the concatenated list) follow in one launch
 * each.  match_cur[k*Cur->n + i2] = position in job k's part of slot[] (0 = offsets[k]) or -1; n_matches[k].  Equal to K
 * calls of orbfe_search_by_projection_keyframe fed with orbfe_project_keyframe's outputs and the table's descriptors, bit for
 * bit.  pose[k].n_levels must not exceed n_levels. */
int orbfe_search_keyframe_mappoints_multi(orbfe_mappoints *mp, const orbfe_frame_view *Cur, const float *scale_factors,
                                          int n_levels, int n_candidates, const int32_t *offsets, const int32_t *slot,
                                          const uint8_t *skip, const float *kf_angle, const orbfe_camera_pose *pose,
                                          const uint8_t *const *blocked, const float *th, const int32_t *orb_dist,
                                          int check_orientation, int32_t *match_cur, int32_t *n_matches);

/* ------------------------------------------------------------------------- */
/* Optimizer::PoseOptimization (src/Optimizer.cc:256-473)                     */
/* ------------------------------------------------------------------------- */
/* The pose-only optimisation Tracking runs between its searches, as ONE kernel launch: the four rounds of up to ten
 * Levenberg iterations with up to ten lambda trials each, on the one graph PoseOptimization builds (one free SE3 vertex,
 * unary mono / stereo reprojection edges, Huber kernel, dense 6 x 6 system).  Not a g2o port: the other Optimizer functions
 * are not covered.  Arithmetic is binary64 as in g2o; inputs are widened from float.  Edge i: xw = GetWorldPos(), (u, v) =
 * mvKeysUn[i].pt, u_right = mvuRight[i] (< 0: a monocular edge), inv_sigma2 = mvInvLevelSigma2[octave]; K5 = fx fy cx cy mbf;
 * Tcw_in = mTcw (row-major 4 x 4).  Outputs: Tcw_out = the pose Frame::SetPose receives, outlier[i] = mvbOutlier,
 * *n_inliers = the return value nInitialCorrespondences - nBad.  With fewer than 3 edges *n_inliers = 0, Tcw_out = Tcw_in
 * and outlier[] is not written (the reference has cleared those mvbOutlier entries by then, :310 / :344; here the caller's
 * array is left alone).  stats (may be NULL): rounds run, and per round the iterations, the lambda trials, the last lambda
 * and the robust chi2 of the estimate.  edge_chi2 (may be NULL): the chi2 each edge was classified with in the last round
 * -- for an inlier that of the last evaluated trial, as g2o leaves it in _error.
 * Sums over edges run in a fixed order that depends on the edge count alone, so equal inputs give equal bits; against g2o
 * they differ by reordering and by the last place of sin / cos.  The 6 x 6 solve is an unpivoted LDL^T.
 * n < 0, n > 16384 (per problem), NULL arrays and offsets that descend return ORBFE_ERR_INVALID before anything is
 * enqueued.  Runs on the calling thread's matcher stream and is complete on return. */
typedef struct orbfe_poseopt_stats {
  int32_t rounds, iterations[4], trials[4];
  double lambda[4], chi2[4];
} orbfe_poseopt_stats;
int orbfe_pose_optimization(int device, int n, const float *xw /*[n,3]*/, const float *u, const float *v,
                            const float *u_right, const float *inv_sigma2, const float K5[5], const float Tcw_in[16],
                            float Tcw_out[16], uint8_t *outlier, int32_t *n_inliers, orbfe_poseopt_stats *stats,
                            double *edge_chi2);
/* n_problems independent problems (one per Relocalization candidate) in one launch, one workgroup each: problem p owns
 * edges [offsets[p], offsets[p+1]) of the edge arrays, K5[5p ..], Tcw_in / Tcw_out[16p ..], n_inliers[p], stats[p].
 * Equal to n_problems single calls, bit for bit. */
int orbfe_pose_optimization_batch(int device, int n_problems, const int32_t *offsets /*[n_problems+1]*/, const float *xw,
                                  const float *u, const float *v, const float *u_right, const float *inv_sigma2,
                                  const float *K5, const float *Tcw_in, float *Tcw_out, uint8_t *outlier,
                                  int32_t *n_inliers, orbfe_poseopt_stats *stats, double *edge_chi2);
/* The same on the resident map-point table, fed with what orbfe_search_local_points returned: feature i of F has an edge
 * when match[i] >= 0 (a position in slot[]) and that slot is not ORBFE_MP_BAD (src/Optimizer.cc:303) -- such a feature is
 * not counted and keeps its flag, as one without a match does.  World positions are gathered from the table on the
 * device; inv_level_sigma2[n_levels] = mvInvLevelSigma2, indexed by F->octave.  The slot list, match[], the frame's
 * keypoint arrays (x, y, octave, u_right; F->u_right NULL: every edge monocular), the level table and the pose go up.
 * outlier / edge_chi2 hold F->n entries.  Equal to orbfe_pose_optimization on the same edges, bit for bit.  Under the
 * handle's serialisation, as the other orbfe_mappoints calls.  A slot outside the table, a match outside slot[] and an
 * octave outside the level table return ORBFE_ERR_INVALID before anything is enqueued. */
int orbfe_pose_optimization_mappoints(orbfe_mappoints *mp, int n_slots, const int32_t *slot, const orbfe_frame_view *F,
                                      const int32_t *match, const float *inv_level_sigma2, int n_levels,
                                      const float K5[5], const float Tcw_in[16], float Tcw_out[16], uint8_t *outlier,
                                      int32_t *n_inliers, orbfe_poseopt_stats *stats, double *edge_chi2);

/* The FeatureVector searches on resident frames (uploaded WITH their FeatureVector and angles): per call only the
 * shared-node list, the MapPoint masks and the result travel.  Semantics and outputs of orbfe_search_by_bow /
 * orbfe_search_by_bow_kf. */
int orbfe_search_by_bow_resident(const orbfe_frame *kf, const uint8_t *has_mp_kf, const orbfe_frame *f, float nnratio,
                                 int check_orientation, int32_t *match_f);
int orbfe_search_by_bow_kf_resident(const orbfe_frame *kf1, const uint8_t *has_mp1, const orbfe_frame *kf2,
                                    const uint8_t *has_mp2, float nnratio, int check_orientation, int32_t *match12);
/* SearchByBoW against n_keyframes candidates in ONE call (one upload of the K shared-node lists and masks, K + 1
 * launches on one stream, one download):
 *   orbfe_search_by_bow_multi:    Tracking::Relocalization, src/Tracking.cc:1478-1498 -- SearchByBoW(pKF_k, mCurrentFrame,
 *       vvpMapPointMatches[k]) for every candidate key frame; match_f [k * f->n + i2] = feature of key frame k matched to
 *       feature i2 of the frame, or -1; n_matches [k];
 *   orbfe_search_by_bow_kf_multi: LoopClosing::ComputeSim3, src/LoopClosing.cc:294-321 -- SearchByBoW(mpCurrentKF, pKF_k,
 *       vvpMapPointMatches[k]); match12 [k * kf1->n + i1] = feature of candidate k matched to feature i1 of kf1, or -1.
 * Every output equals the corresponding single-pair call. */
int orbfe_search_by_bow_multi(int n_keyframes, const orbfe_frame *const *kf, const uint8_t *const *has_mp_kf,
                              const orbfe_frame *f, float nnratio, int check_orientation, int32_t *match_f,
                              int32_t *n_matches);
int orbfe_search_by_bow_kf_multi(const orbfe_frame *kf1, const uint8_t *has_mp1, int n_keyframes,
                                 const orbfe_frame *const *kf2, const uint8_t *const *has_mp2, float nnratio,
                                 int check_orientation, int32_t *match12, int32_t *n_matches);
/* ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:754-928) of ONE key frame against n_neighbours key frames in
 * one call -- the loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:283-315): F12[9*k ..], ex[k], ey[k]
 * the fundamental matrix and epipole of neighbour k, has_mp2[k] its MapPoint mask; the stereo flags come from the
 * frames' u_right.  match12[k*n1 + i] = feature of neighbour k matched to feature i of kf1, or -1; n_matches[k].
 * One upload, 2 launches per neighbour on one stream, one download. */
int orbfe_search_for_triangulation_multi(const orbfe_frame *kf1, const uint8_t *has_mp1, int n_neighbours,
                                         const orbfe_frame *const *kf2, const uint8_t *const *has_mp2,
                                         const float *F12, const float *ex, const float *ey,
                                         const float *scale_factors2, const float *level_sigma2_2, int n_levels2,
                                         int only_stereo, int check_orientation, int32_t *match12,
                                         int32_t *n_matches);
/* The per-point search of ORBmatcher::Fuse (orbfe_fuse_search) for the SAME n map points against n_keyframes key
 * frames in one call -- LocalMapping::SearchInNeighbors (src/LocalMapping.cc:542-549).  valid / u / v / ur / level /
 * best_idx are [k*n + i]; mp_desc [n*32] is shared; resident views upload nothing of the key frames. */
int orbfe_fuse_search_multi(int device, int n_keyframes, const orbfe_frame_view *const *KF,
                            const float *scale_factors, const float *inv_level_sigma2, int n_levels, int n,
                            const uint8_t *valid, const float *u, const float *v, const float *ur,
                            const int32_t *level, const uint8_t *mp_desc, float th, int chi2_gate,
                            int32_t *best_idx);

/* LocalMapping::CreateNewMapPoints, the per-pair loop between the two calls above (src/LocalMapping.cc:331-501): the
 * parallax test, the 4 x 4 linear triangulation or KeyFrame::UnprojectStereo, the positive-depth test in both cameras, the
 * two reprojection gates and the scale-consistency test, for every matched pair of ONE key frame against n_neighbours key
 * frames as ONE kernel launch, one lane per pair.  match12 [k*n1 + i1] is what orbfe_search_for_triangulation_multi
 * returned (feature of neighbour k or -1); cam1 / cam2[k] hold what the loop reads of the key frames besides their
 * keypoints; scale_factors / level_sigma2 [n_levels] = mvScaleFactors / mvLevelSigma2 (shared by all key frames, as the
 * reference's are); ratio_factor = 1.5f * mfScaleFactor (:278).
 * Arithmetic is binary64 on inputs widened from float, in a fixed order, so equal inputs give equal bits.  The null vector of
 * the 4 x 4 system comes from a one-sided Jacobi SVD (fixed pair order, at most 30 sweeps, a rotation skipped when
 * |a_p.a_q| <= DBL_EPSILON sqrt(|a_p|^2 |a_q|^2)).  The reference computes in CV_32F with cv::SVD: results agree with it to
 * float rounding and are NOT bit-identical to it; a pair within float rounding of a gate may fall on the other side.  Kept
 * as the reference has them: the `else if` of :358-361 (key frame 2's stereo parallax only when keypoint 1 is monocular),
 * the double literals 0.9998 / 5.991 / 7.8, key frame 1's mbf in the SECOND reprojection gate (:455), the raw keypoint
 * position in UnprojectStereo (src/KeyFrame.cc:663-664).
 * Outputs, [k*n1 + i1] as match12: status = ORBFE_TRI_NO_MATCH where match12 is -1, else ORBFE_TRI_CREATED or the
 * `continue` the pair left the loop by; x3d [3 * slot ..] = the new point (binary64 result rounded once) where status is
 * CREATED, zeros elsewhere; n_created[k] = CREATED pairs of neighbour k; winner[i1] = the smallest k whose pair for keypoint
 * i1 is CREATED, or -1.
 * What winner is for: the reference gives keypoint i1 its MapPoint at the FIRST neighbour that succeeds (AddMapPoint, :489)
 * and no longer searches i1 for later neighbours (src/ORBmatcher.cc:800-803).  With the multi search every neighbour was
 * searched with the mask of entry, so the caller replays the neighbours in order and keeps, for each i1, only the pair with
 * k == winner[i1].  What remains different: in the reference, masking i1 could free its idx2 for another keypoint of the
 * same neighbour; that is a deviation of orbfe_search_for_triangulation_multi, not of this call.
 * Views with `resident` set upload nothing of the frame, host views upload x / y / octave / u_right; per call the pair
 * records, the K + 1 cameras and the level tables go up and the four outputs come back in one copy.  n_neighbours outside
 * [0, 64], more than 16384 keypoints, a match outside [-1, n2), a matched keypoint's octave outside [0, n_levels), n_levels
 * outside (0, ORBFE_MAX_LEVELS], a matched stereo keypoint (u_right >= 0) without `depth` or with a depth <= 0 (the reference
 * would dereference an empty matrix there) and NULL arrays return ORBFE_ERR_INVALID before anything is enqueued.
 * n_neighbours = 0, or no pair at all, returns ORBFE_OK with the outputs initialised and no launch.  Runs on the calling
 * thread's matcher stream and is complete on return. */
typedef struct orbfe_keyframe_camera {   /* a key frame as CreateNewMapPoints reads it */
  float Tcw[12];                         /* [Rcw | tcw], row-major 3 x 4 (GetRotation / GetTranslation) */
  float Ow[3];                           /* GetCameraCenter() */
  float fx, fy, cx, cy, invfx, invfy, mb, mbf;
  const float *depth;                    /* mvDepth [n], NULL: no stereo keypoints are unprojected (monocular) */
  const float *x_raw, *y_raw;            /* mvKeys[i].pt for UnprojectStereo, NULL: the view's x / y (mvKeys == mvKeysUn:
                                            every camera without distortion, src/Frame.cc:445-449) */
} orbfe_keyframe_camera;

enum { ORBFE_TRI_NO_MATCH = 0, ORBFE_TRI_CREATED = 1, ORBFE_TRI_LOW_PARALLAX, ORBFE_TRI_W_ZERO, ORBFE_TRI_BEHIND_1,
       ORBFE_TRI_BEHIND_2, ORBFE_TRI_REPROJ_1, ORBFE_TRI_REPROJ_2, ORBFE_TRI_DIST_ZERO, ORBFE_TRI_SCALE };

int orbfe_triangulate_matches_multi(int device, const orbfe_frame_view *KF1, const orbfe_keyframe_camera *cam1,
                                    int n_neighbours, const orbfe_frame_view *const *KF2,
                                    const orbfe_keyframe_camera *cam2 /*[K]*/, const int32_t *match12 /*[K*n1]*/,
                                    const float *scale_factors, const float *level_sigma2, int n_levels,
                                    float ratio_factor, float *x3d /*[K*n1*3]*/, uint8_t *status /*[K*n1]*/,
                                    int32_t *n_created /*[K]*/, int32_t *winner /*[n1]*/);
/* One neighbour (match12 [n1], n_created [1]); equal to the multi form with n_neighbours = 1, without winner. */
int orbfe_triangulate_matches(int device, const orbfe_frame_view *KF1, const orbfe_keyframe_camera *cam1,
                              const orbfe_frame_view *KF2, const orbfe_keyframe_camera *cam2, const int32_t *match12,
                              const float *scale_factors, const float *level_sigma2, int n_levels, float ratio_factor,
                              float *x3d, uint8_t *status, int32_t *n_created);

/* Sim3Solver (src/Sim3Solver.cc), the RANSAC between SearchByBoW and SearchBySim3 in LoopClosing::ComputeSim3
 * (src/LoopClosing.cc:286-404): EVERY hypothesis of EVERY candidate's solver in ONE kernel launch, one wave per hypothesis.
 * A hypothesis is Sim3Solver::ComputeSim3 (:254-370, Horn's closed form) on three matched pairs followed by CheckInliers
 * (:374-398) over all pairs of its candidate.  Hypotheses are independent; the order-dependent part of iterate() (:150-220:
 * best on >=, return on > minInliers) is a scan over n_inliers that the caller replays on the host (C++
 * orbfe_cpp::Sim3Solver, Python Sim3Solver).
 * Candidate k owns pairs [pair_off[k], pair_off[k+1]) of x3dc1 / x3dc2 (mvX3Dc1 / mvX3Dc2, :95-98: the matched MapPoints in
 * the cameras of key frames 1 and 2) and of max_err1 / max_err2 (mvnMaxError1 / 2 = 9.210 * sigma2, :87-88), the cameras
 * cam1[k] / cam2[k] = fx fy cx cy of mK1 / mK2, and hypotheses [hyp_off[k], hyp_off[k+1]); triples[3 h ..] are the three
 * pairs of hypothesis h as indices LOCAL to its candidate's pairs (what :176-187 draws).  fix_scale = mbFixScale.
 * Arithmetic is binary64 on inputs widened from float, in a fixed order, so equal inputs give equal bytes.  The eigenvector
 * of N comes from a cyclic Jacobi iteration (fixed pair order, at most 30 sweeps, a rotation skipped when
 * |a_pq| <= DBL_EPSILON sqrt(|a_pp a_qq|)), the rotation from it the reference's way (angle-axis, cv::Rodrigues' formula).
 * The reference computes in CV_32F with cv::eigen / cv::Rodrigues: results agree with it to float rounding and are NOT
 * bit-identical to it; a pair within float rounding of its max_err may fall on the other side.  Kept as the reference has
 * them: no depth test in Project (:436), strict < in :390, and the division by |vec| = 0 of :310 for two identical triples,
 * after which everything is NaN and no pair is an inlier.
 * Outputs per hypothesis h: n_inliers[h]; status[h] = ORBFE_SIM3_OK, or ORBFE_SIM3_NONFINITE when any of R, t, s is not finite
 * (n_inliers 0 and all mask words 0 then; R, t, s stored as they came out); sim3[13 h ..] = R12 row-major, t12, s12 (binary64
 * results rounded once); its ceil(n_k / 32) mask words at mask_words[word_off[k] + (h - hyp_off[k]) * ceil(n_k / 32)], pair i
 * of the candidate at bit i & 31 of word i >> 5.  word_off [K + 1] is written by the call; mask_words must hold
 * sum_k H_k * ceil(n_k / 32) words.
 * Returns ORBFE_ERR_INVALID before anything is enqueued, leaving the thread usable, for: NULL arrays, offsets that do not
 * start at 0, decrease, or do not end at n_pairs / n_hypotheses, a triple index outside [0, n_k), a triple that repeats an
 * index, a camera entry that is not finite, a candidate with n_k < 3 that has hypotheses, n_candidates outside [0, 4096].
 * A candidate without hypotheses is legal; a call without any returns ORBFE_OK with word_off written and no launch.  Runs on
 * the calling thread's matcher stream and is complete on return. */
enum { ORBFE_SIM3_OK = 0, ORBFE_SIM3_NONFINITE = 1 };

int orbfe_sim3_ransac_multi(int device, int n_candidates, int n_pairs, int n_hypotheses, const int32_t *pair_off /*[K+1]*/,
                            const float *x3dc1 /*[N*3]*/, const float *x3dc2 /*[N*3]*/, const float *max_err1 /*[N]*/,
                            const float *max_err2 /*[N]*/, const float *cam1 /*[K*4]*/, const float *cam2 /*[K*4]*/,
                            int fix_scale, const int32_t *hyp_off /*[K+1]*/, const int32_t *triples /*[H*3]*/,
                            int32_t *n_inliers /*[H]*/, uint8_t *status /*[H]*/, float *sim3 /*[H*13]*/,
                            uint32_t *mask_words, int32_t *word_off /*[K+1]*/);
/* One candidate; equal to the multi form with n_candidates = 1.  mask_words [H * ceil(n / 32)]. */
int orbfe_sim3_ransac(int device, int n_pairs, const float *x3dc1, const float *x3dc2, const float *max_err1,
                      const float *max_err2, const float *cam1, const float *cam2, int fix_scale, int n_hypotheses,
                      const int32_t *triples, int32_t *n_inliers, uint8_t *status, float *sim3, uint32_t *mask_words);
/* The selection without replacement of Sim3Solver::iterate (:173-187), no device involved: draws[3 h + i] is the value
 * RandomInt(0, vAvailableIndices.size() - 1) returned for pick i of hypothesis h, in [0, n - 1 - i] -- an index INTO the list
 * of still available pairs, which starts as 0 .. n-1 for every hypothesis and loses the pair taken by swap-with-back and pop
 * -> triples[3 h + i] the pair taken.  A caller who feeds the reference's DUtils::Random::RandomInt stream gets the
 * reference's triples; the library does not restate rand().  n < 3 with hypotheses, NULL arrays or a draw outside its range
 * return ORBFE_ERR_INVALID. */
int orbfe_sim3_triples_from_draws(int n, int n_hypotheses, const int32_t *draws /*[H*3]*/, int32_t *triples /*[H*3]*/);
/* What Sim3Solver::SetRansacParameters (:118-142) leaves in mRansacMaxIts for n correspondences: the reference's float
 * epsilon = minInliers / n, ceil(log(1 - prob) / log(1 - pow(epsilon, 3))), max(1, min(., max_its)), 1 when
 * min_inliers == n.  n < min_inliers returns 1 without the formula (the reference's expression is NaN there and iterate()
 * never reads the result). */
int orbfe_sim3_max_iterations(int n, double prob, int min_inliers, int max_its);

/* PnPsolver (src/PnPsolver.cc), the RANSAC of Tracking::Relocalization (src/Tracking.cc:1487-1560) between SearchByBoW and
 * PoseOptimization: EVERY hypothesis of EVERY candidate's solver in ONE kernel launch, one wave per hypothesis, and every
 * Refine() problem of every candidate in a second one, one workgroup per problem.  A hypothesis is compute_pose (:544-598,
 * EPnP) on four correspondences followed by CheckInliers (:323-354) over all correspondences of its candidate.  Refine()
 * (:275-320) is compute_pose on the correspondences of a best inlier set, then CheckInliers.  It is a pure function of that
 * set, and the set changes only where a hypothesis has n_inliers >= minInliers and more inliers than every earlier such
 * hypothesis: those hypotheses are the Refine records of a solver.  The order-dependent rest of iterate() (:178-271) is a
 * scan over the two result sets that the caller replays on the host (C++ orbfe_cpp::PnPsolver, Python PnPsolver).
 * Candidate k owns correspondences [point_off[k], point_off[k+1]) of p3d (mvP3Dw), p2d (mvP2D) and max_err2 (mvMaxError =
 * sigma2 * th2, :163), the camera cam[k] = fu fv uc vc, and hypotheses [hyp_off[k], hyp_off[k+1]); sets[4 h ..] are the four
 * correspondences of hypothesis h as indices LOCAL to its candidate (what :204-214 draws).
 * Arithmetic is binary64 on inputs widened from float, in a fixed order, so equal inputs give equal bytes; CheckInliers has
 * the reference's own float / double mix and strict <.  Two DEVIATIONS from the reference, whose decompositions are
 * OpenCV's and so depend on the OpenCV build:
 *   - the decompositions are Jacobi iterations (3 x 3 SVDs, the least squares of find_betas_approx_*, the eigenvectors of
 *     the 12 x 12 M^T M: fixed pair order, at most 30 sweeps, a rotation skipped when |a_pq| <= DBL_EPSILON sqrt(|a_pp a_qq|));
 *     the rows of UCt in choose_control_points are signed so that their largest component is positive.  Results agree with
 *     cv::SVD to rounding and are NOT bit-identical to it;
 *   - for FOUR correspondences M is 8 x 12 and EPnP takes four vectors of a null space of dimension >= 4, inside which an
 *     eigen-solver's basis is rounding noise.  The basis is canonical here: Householder QR of M^T, reflector k mapping its
 *     column to -sign(alpha) |x| e_1 with sign(0) = +1, ut rows 8 .. 11 = Q e_8 .. Q e_11.  It spans the same subspace as the
 *     reference's four vectors and is a continuous function of M wherever M has rank 8.
 * Outputs per hypothesis or record h: n_inliers[h]; status[h] = ORBFE_PNP_OK, or ORBFE_PNP_NONFINITE when any entry of R or
 * t is not finite (n_inliers 0 and all mask words 0 then); pose[12 h ..] = R row-major, then t (binary64 results rounded
 * once: what mBestTcw / mRefinedTcw hold); its ceil(n_k / 32) mask words at
 * mask_words[word_off[k] + (h - hyp_off[k]) * ceil(n_k / 32)], correspondence i at bit i & 31 of word i >> 5.  word_off
 * [K + 1] is written by the call; mask_words must hold sum_k H_k * ceil(n_k / 32) words.
 * Returns ORBFE_ERR_INVALID before anything is enqueued, leaving the thread usable, for: NULL arrays, offsets that do not
 * start at 0, decrease, or do not end at the totals, a set index outside [0, n_k) or repeated within a set, a camera entry
 * that is not finite, a candidate with n_k < 4 that has hypotheses or records, a record mask with fewer than 4 bits or with
 * bits at or beyond n_k, n_candidates outside [0, 4096].  A candidate without hypotheses is legal; a call without any returns
 * ORBFE_OK with word_off written and no launch.  Runs on the calling thread's matcher stream and is complete on return. */
enum { ORBFE_PNP_OK = 0, ORBFE_PNP_NONFINITE = 1 };

int orbfe_pnp_ransac_multi(int device, int n_candidates, int n_points, int n_hypotheses, const int32_t *point_off /*[K+1]*/,
                           const float *p3d /*[N*3]*/, const float *p2d /*[N*2]*/, const float *max_err2 /*[N]*/,
                           const float *cam /*[K*4]*/, const int32_t *hyp_off /*[K+1]*/, const int32_t *sets /*[H*4]*/,
                           int32_t *n_inliers /*[H]*/, uint8_t *status /*[H]*/, float *pose /*[H*12]*/,
                           int32_t *word_off /*[K+1]*/, uint32_t *mask_words);
/* One candidate; equal to the multi form with n_candidates = 1.  mask_words [H * ceil(n / 32)]. */
int orbfe_pnp_ransac(int device, int n_points, const float *p3d, const float *p2d, const float *max_err2, const float *cam,
                     int n_hypotheses, const int32_t *sets, int32_t *n_inliers, uint8_t *status, float *pose,
                     uint32_t *mask_words);
/* The Refine() problems: candidate k owns records [rec_off[k], rec_off[k+1]); rec_masks holds ceil(n_k / 32) words per
 * record, candidate after candidate (the layout mask_words has): the correspondences EPnP runs on, in index order.  Outputs
 * as above, per record. */
int orbfe_pnp_refine_multi(int device, int n_candidates, int n_points, int n_records, const int32_t *point_off /*[K+1]*/,
                           const float *p3d, const float *p2d, const float *max_err2, const float *cam,
                           const int32_t *rec_off /*[K+1]*/, const uint32_t *rec_masks, int32_t *n_inliers /*[R]*/,
                           uint8_t *status /*[R]*/, float *pose /*[R*12]*/, int32_t *word_off /*[K+1]*/, uint32_t *mask_words);
/* Both launches and the record scan between them: the hypotheses as orbfe_pnp_ransac_multi, then for candidate k with
 * min_inliers[k] (mRansacMinInliers after SetRansacParameters, >= 4) the records rec_hyp[rec_off[k] .. rec_off[k+1]) = the
 * hypotheses (indices into the call's H) whose n_inliers is >= min_inliers[k] and above every earlier such count, and the
 * results of Refine() on their masks.  The rec_* arrays must hold what H records need (rec_mask_words as many words as
 * mask_words). */
int orbfe_pnp_solve_multi(int device, int n_candidates, int n_points, int n_hypotheses, const int32_t *point_off,
                          const float *p3d, const float *p2d, const float *max_err2, const float *cam, const int32_t *hyp_off,
                          const int32_t *sets, const int32_t *min_inliers /*[K]*/, int32_t *n_inliers, uint8_t *status,
                          float *pose, int32_t *word_off, uint32_t *mask_words, int32_t *rec_off /*[K+1]*/,
                          int32_t *rec_hyp, int32_t *rec_n_inliers, uint8_t *rec_status, float *rec_pose,
                          int32_t *rec_word_off /*[K+1]*/, uint32_t *rec_mask_words);
/* The selection without replacement of PnPsolver::iterate (:201-214), no device involved: draws[4 h + i] is the value
 * RandomInt(0, vAvailableIndices.size() - 1) returned for pick i of hypothesis h, in [0, n - 1 - i] -- an index INTO the list
 * of still available correspondences, which starts as 0 .. n-1 for every hypothesis and loses the entry taken by
 * swap-with-back and pop -> sets[4 h + i] the correspondence taken.  A caller who feeds the reference's
 * DUtils::Random::RandomInt stream gets the reference's sets; the library does not restate rand().  n < 4 with hypotheses,
 * NULL arrays or a draw outside its range return ORBFE_ERR_INVALID. */
int orbfe_pnp_sets_from_draws(int n, int n_hypotheses, const int32_t *draws /*[H*4]*/, int32_t *sets /*[H*4]*/);

/* -------------------------------------------------------------------------- */
/* Initializer::FindHomography / FindFundamental (src/Initializer.cc:141-255)  */
/* -------------------------------------------------------------------------- */
/* The RANSAC of monocular map initialisation, the step after SearchForInitialization in Tracking::MonocularInitialization:
 * EVERY hypothesis of BOTH models of EVERY problem in ONE kernel launch, one wave per (set, model).  A hypothesis is the
 * normalised 8-point DLT of ComputeH21 (:260-305) or ComputeF21 (:307-345, with the rank-2 step) on the 8 pairs of a set,
 * un-normalised (:187-188, :244), followed by CheckHomography (:350-436) or CheckFundamental (:444-526) over all pairs of its
 * problem.  Hypotheses are independent; the order-dependent part (`currentScore > score`, :192, :248) is a scan over the
 * scores that the caller replays on the host (include/orbfe_initializer_replay.hpp, C++ orbfe_cpp::Initializer, Python
 * Initializer).
 * Problem k owns pairs [pair_off[k], pair_off[k+1]) of pairs[4 i ..] = u1 v1 u2 v2 (mvKeys1[mvMatches12[i].first].pt,
 * mvKeys2[mvMatches12[i].second].pt), T1[4 k ..] / T2[4 k ..] = sX sY meanX meanY of Normalize over ALL keys of frame 1 / 2
 * (orbfe_initializer_normalize), sigma[k] = mSigma and sets [hyp_off[k], hyp_off[k+1]); sets[8 h ..] are the 8 pairs of set h
 * (mvSets[h]) as indices LOCAL to its problem's pairs.  Both models use the same sets.
 * Arithmetic is binary64 on inputs widened from float, in a fixed order, so equal inputs give equal bytes.  The null vector
 * of the 16 x 9 / 8 x 9 matrix comes from a one-sided (Hestenes) Jacobi iteration on its columns (pair order (0,1) ... (7,8),
 * at most 30 sweeps, a rotation skipped when |a_p . a_q| <= DBL_EPSILON |a_p| |a_q|); it is the column of V under the column
 * of the smallest norm.  The reference computes in CV_32F with cv::SVDecomp: results agree with it to float rounding and are
 * NOT bit-identical to it; a pair within float rounding of a threshold may fall on the other side.  Kept as the reference
 * has them: cv::Mat::inv() of a singular H21 is the zero matrix, every chi-square is then NaN, takes the else branch of
 * `if (chi > th)` and makes the score NaN.
 * Outputs per (set h, model m), m = ORBFE_INIT_MODEL_H or _F, at index g = 2 h + m: score[g] (the float score of the
 * reference, in binary64); status[g] = ORBFE_INIT_OK, or ORBFE_INIT_NONFINITE when the score or an entry of the model (or of
 * H12) is not finite (n_inliers 0 and all mask words 0 then; score and model stored as they came out: `score > best` is false
 * for it); n_inliers[g]; model[9 g ..] = H21 or F21 row-major; h12[9 h ..] = H12 of set h; its ceil(n_k / 32) mask words at
 * mask_words[word_off[k] + (2 (h - hyp_off[k]) + m) * ceil(n_k / 32)], pair i of the problem at bit i & 31 of word i >> 5.
 * word_off [K + 1] is written by the call; mask_words must hold sum_k 2 H_k ceil(n_k / 32) words.
 * Returns ORBFE_ERR_INVALID before anything is enqueued, leaving the thread usable, for: NULL arrays, offsets that do not
 * start at 0, decrease, or do not end at n_pairs / n_sets, a set index outside [0, n_k), a set that repeats an index, a
 * problem with n_k < 8 that has sets, an entry of T1 / T2 or a sigma that is not finite, sigma <= 0, n_problems outside
 * [0, 4096], more than 2^24 sets.  A problem without pairs and sets is legal; a call without any set returns ORBFE_OK with
 * word_off written and no launch.  Runs on the calling thread's matcher stream and is complete on return. */
enum { ORBFE_INIT_OK = 0, ORBFE_INIT_NONFINITE = 1 };
enum { ORBFE_INIT_MODEL_H = 0, ORBFE_INIT_MODEL_F = 1 };

int orbfe_initializer_ransac_multi(int device, int n_problems, int n_pairs, int n_sets, const int32_t *pair_off /*[K+1]*/,
                                   const float *pairs /*[N*4]*/, const double *T1 /*[K*4]*/, const double *T2 /*[K*4]*/,
                                   const float *sigma /*[K]*/, const int32_t *hyp_off /*[K+1]*/, const int32_t *sets /*[H*8]*/,
                                   double *score /*[H*2]*/, uint8_t *status /*[H*2]*/, int32_t *n_inliers /*[H*2]*/,
                                   double *model /*[H*2*9]*/, double *h12 /*[H*9]*/, uint32_t *mask_words,
                                   int32_t *word_off /*[K+1]*/);
/* One problem; equal to the multi form with n_problems = 1.  mask_words [H * 2 * ceil(n / 32)]. */
int orbfe_initializer_ransac(int device, int n_pairs, const float *pairs, const double *T1 /*[4]*/, const double *T2 /*[4]*/,
                             float sigma, int n_sets, const int32_t *sets, double *score, uint8_t *status, int32_t *n_inliers,
                             double *model, double *h12, uint32_t *mask_words);
/* Initializer::Normalize (:852-904) over ALL n_keys undistorted keys of a frame (keys_xy = x y interleaved), as :149-150
 * call it -- not only the matched ones -> T = sX sY meanX meanY.  Host code, binary64, sequential sums in index order (the
 * reference sums in float).  n_keys <= 0 or a NULL array return ORBFE_ERR_INVALID. */
int orbfe_initializer_normalize(int n_keys, const float *keys_xy /*[n*2]*/, double *T /*[4]*/);
/* The selection without replacement of Initializer::Initialize (:93-108), no device involved: draws[8 h + j] is the value
 * RandomInt(0, vAvailableIndices.size() - 1) returned for pick j of set h, in [0, n - j) -- an index INTO the list of still
 * available pairs, which starts as 0 .. n-1 for every set and loses the pair taken by swap-with-back and pop -> sets[8 h + j]
 * the pair taken.  A caller who feeds the reference's DUtils::Random::RandomInt stream gets the reference's mvSets; the
 * library does not restate rand().  n < 8 with sets, NULL arrays or a draw outside its range return ORBFE_ERR_INVALID. */
int orbfe_initializer_sets_from_draws(int n, int n_sets, const int32_t *draws /*[H*8]*/, int32_t *sets /*[H*8]*/);

/* Initializer::ReconstructH (:653-824) / ReconstructF (:536-642) up to their order-dependent tails: what Initialize does with
 * the chosen model.  ONE kernel launch, one workgroup of 256 lanes per (problem, hypothesis): the 8 motion hypotheses of an H
 * problem (Faugeras, :667-775, in the reference's index order: 0-3 the case d' = d2, 4-7 the case d' = -d2) or the 4 of an F
 * problem ((R1,t) (R2,t) (R1,-t) (R2,-t) of DecomposeE, :546-566, :1034-1057), and for each of them CheckRT (:913-1029) over
 * the problem's inlier pairs.  The tails (:568-641, :778-823) are replayed on the host from n_good and cos_sel
 * (include/orbfe_initializer_replay.hpp, C++ orbfe_cpp::Initializer::Reconstruct / Initialize, Python Initializer).
 * Problem k owns pairs [pair_off[k], pair_off[k+1]) (u1 v1 u2 v2 as for orbfe_initializer_ransac*), model_kind[k] =
 * ORBFE_INIT_MODEL_H or _F, model[9 k ..] = H21 or F21 row-major, K4[4 k ..] = fx fy cx cy, sigma[k] = mSigma and the
 * ceil(n_k / 32) words inlier_words[in_word_off[k] ..] = vbMatchesInliers in the mask format of orbfe_initializer_ransac*
 * (pair i at bit i & 31 of word i >> 5; bits past n_k are ignored).  in_word_off[k+1] - in_word_off[k] must be ceil(n_k / 32).
 * Arithmetic is binary64 on inputs widened from float, in a fixed order: equal inputs give equal bytes, and the multi form
 * equals the single calls byte for byte.  K.inv() is its closed form.  The 3 x 3 SVD (of K^-1 H21 K, :673; of K^T F21 K,
 * :1037) is a one-sided Jacobi iteration on the columns (pair order (0,1) (0,2) (1,2), a rotation skipped when
 * |a_p . a_q| <= DBL_EPSILON |a_p| |a_q|, at most 30 sweeps), singular values descending, u_i = A v_i / w_i for i = 0, 1 and
 * u_2 = +-(u_0 x u_1) with the sign of (u_0 x u_1) . (A v_2), + when that is 0 -- E21 has rank 2, a normalised A v_2 would be
 * noise.  The signs of the singular vectors are free as in any SVD and permute the hypotheses among themselves (H: 0 <-> 2,
 * 1 <-> 3 within each group of four; F: t <-> -t, R1 <-> R2).  The 4 x 4 null vector of Triangulate (:829-842) is the Jacobi
 * routine of orbfe_triangulate_new_points.  The reference computes in CV_32F with cv::SVD: results agree with it to float
 * rounding and are NOT bit-identical to the CV_32F cv::SVD path; a pair within float rounding of a threshold may fall on the
 * other side.  Every comparison is written as the reference writes it (`!isfinite`, `z <= 0 && cos < 0.99998` twice,
 * `squareError > th2` twice with th2 = 4 sigma^2), so NaN takes the reference's branches.
 * An H problem whose singular values meet `d1/d2 < 1.00001 || d2/d3 < 1.00001` (:684, as written: a NaN or inf ratio does not)
 * has problem_status ORBFE_RECON_DEGENERATE: its 8 slots stay, with R, t, the points and the flags zero and every n_good 0.
 * Written by the call: hyp_off [K+1] (8 per H problem, 4 per F problem) and slot_off [K+1] (slot_off[k+1] - slot_off[k] =
 * hypotheses of k times n_k).  With G = hyp_off[K] and S = slot_off[K], per hypothesis g: R[9 g ..] row-major, t[3 g ..]
 * (unit), n_good[g] = CheckRT's return value (an integer sum in a fixed tree; no floating-point atomics anywhere), cos_sel[g]
 * = the element at index min(50, n_sel - 1) of the ascending order of the finite cosines of the counted pairs (:1018-1023;
 * found exactly, by bisection on an order-preserving 64-bit key; 0.0 when there is none; the device takes no acos: parallax =
 * acos(cos_sel) 180 / pi belongs to the replay), hyp_status[g] = ORBFE_RECON_OK, or ORBFE_RECON_NONFINITE when a counted pair's
 * cosine is not finite (it counts in n_good and is left out of the selection: the reference sorts a NaN there, which is
 * undefined).  Per (hypothesis g of problem k, pair i of k) at slot s = slot_off[k] + (g - hyp_off[k]) n_k + i: x3d[3 s ..] =
 * the triangulated point in camera 1 as it came out, pair_flags[s] bit 0 = the pair added 1 to n_good, bit 1 = vbGood (bit 0
 * and cos < 0.99998); zero for a pair whose inlier bit is clear.  Per problem: problem_status[k], n_inliers[k] = N of :540-543.
 * Returns ORBFE_ERR_INVALID before anything is enqueued, leaving the thread usable, for: NULL arrays (x3d and pair_flags
 * included, even when S = 0), offsets that do not start at 0, decrease, or do not end at n_pairs / n_words, a problem whose
 * word count is not ceil(n_k / 32), a model kind other than the two, a non-finite entry of model or K4, fx or fy equal to 0, a
 * sigma that is not finite or <= 0, n_problems outside [0, 4096], more than 2^31 - 1 slots.  A problem without pairs or with an
 * all-zero mask is legal (every n_good 0, cos_sel 0.0); a call without problems returns ORBFE_OK without a launch.  Runs on the
 * calling thread's matcher stream and is complete on return. */
enum { ORBFE_RECON_OK = 0, ORBFE_RECON_NONFINITE = 1 };
enum { ORBFE_RECON_PROBLEM_OK = 0, ORBFE_RECON_DEGENERATE = 1 };

int orbfe_initializer_reconstruct_multi(int device, int n_problems, int n_pairs, int n_words, const int32_t *pair_off /*[K+1]*/,
                                        const float *pairs /*[N*4]*/, const int32_t *model_kind /*[K]*/,
                                        const double *model /*[K*9]*/, const float *K4 /*[K*4]*/, const float *sigma /*[K]*/,
                                        const uint32_t *inlier_words /*[W]*/, const int32_t *in_word_off /*[K+1]*/,
                                        int32_t *hyp_off /*[K+1]*/, int32_t *slot_off /*[K+1]*/, double *R /*[G*9]*/,
                                        double *t /*[G*3]*/, int32_t *n_good /*[G]*/, double *cos_sel /*[G]*/,
                                        uint8_t *hyp_status /*[G]*/, double *x3d /*[S*3]*/, uint8_t *pair_flags /*[S]*/,
                                        uint8_t *problem_status /*[K]*/, int32_t *n_inliers /*[K]*/);
/* One problem; equal to the multi form with n_problems = 1.  G = 8 or 4, S = G n_pairs, inlier_words [ceil(n / 32)]. */
int orbfe_initializer_reconstruct(int device, int n_pairs, const float *pairs, int model_kind, const double *model /*[9]*/,
                                  const float *K4 /*[4]*/, float sigma, const uint32_t *inlier_words, double *R, double *t,
                                  int32_t *n_good, double *cos_sel, uint8_t *hyp_status, double *x3d, uint8_t *pair_flags,
                                  uint8_t *problem_status, int32_t *n_inliers);

/* -------------------------------------------------------------------------- */
/* Optimizer::OptimizeSim3 (src/Optimizer.cc:1116-1323)                        */
/* -------------------------------------------------------------------------- */
/* The Sim3 refinement LoopClosing::ComputeSim3 runs on every candidate that survives Sim3Solver and SearchBySim3
 * (src/LoopClosing.cc:387-388), ONE kernel launch per call: both rounds (optimize(5), erase, optimize(5 or 10), erase), their
 * Levenberg iterations with up to ten lambda trials each, and the "fewer than 10 pairs left" exit, on the one graph
 * OptimizeSim3 builds (one free Sim3 vertex S12, per pair an EdgeSim3ProjectXYZ and an EdgeInverseSim3ProjectXYZ with
 * information invSigma2 I and a Huber kernel of delta = sqrt(th2), a dense 7 x 7 system).  Arithmetic is binary64 on inputs
 * widened from float.  g2o differentiates the two edges numerically; the call uses the analytic Jacobian of the same left
 * update, so it agrees with g2o to the accuracy of g2o's difference quotient and is not bit-identical to it.
 * As in the reference, a classification reads the error of the LAST evaluated Levenberg trial, accepted or not.
 * K problems; pair_off[K+1]; per pair: X1 = R1w*P1w+t1w, X2 likewise (float, as cv::Mat holds them), obs1 = mvKeysUn1[i].pt,
 * obs2 = mvKeysUn2[i2].pt, the two mvInvLevelSigma2[octave]; per problem: cam1/cam2 = fx fy cx cy, sim3_in[13] = R row-major, t, s
 * (the layout orbfe_sim3_ransac_multi writes), th2, fix_scale.  sim3_out[8] = qx qy qz qw tx ty tz s: g2o::Sim3's own members.
 * Outputs per problem: n_in (the return value of OptimizeSim3); sim3_out -- the incoming S12 converted as
 * Sim3(Matrix3d, Vector3d, double) does whenever n_in comes from the early return (fewer than 10 pairs left after round
 * one, or no pair at all), the optimised S12 otherwise; bad[i] = 0 kept, 1 erased after round one, 2 erased after round two
 * (the caller sets vpMatches1[idx] = NULL for every bad[i] != 0, also after the early return); chi2_12 / chi2_21 (both may
 * be NULL) the chi2 the last classification of the pair read.  stats may be NULL.
 * Limits: 16384 pairs per problem, 1048576 problems.  Returns ORBFE_ERR_INVALID before anything is enqueued, leaving the
 * thread usable, for: NULL arrays, pair_off that does not start at 0 or descends, a problem above the limit, a th2 that is
 * not positive and finite.  Runs on the calling thread's matcher stream and is complete on return. */
typedef struct orbfe_optsim3_stats { int32_t rounds, n_bad; int32_t iterations[2], trials[2]; double lambda[2], chi2[2]; } orbfe_optsim3_stats;
int orbfe_optimize_sim3_multi(int device, int n_problems, const int32_t *pair_off, const float *x3dc1, const float *x3dc2,
                              const float *obs1, const float *obs2, const float *inv_sigma2_1, const float *inv_sigma2_2,
                              const float *cam1, const float *cam2, const float *sim3_in, const float *th2, const uint8_t *fix_scale,
                              double *sim3_out, uint8_t *bad, int32_t *n_in, orbfe_optsim3_stats *stats,
                              double *chi2_12, double *chi2_21 /* both may be NULL */);
/* One problem; bit-equal to the multi form with n_problems = 1. */
int orbfe_optimize_sim3(int device, int n, const float *x3dc1, const float *x3dc2, const float *obs1, const float *obs2,
                        const float *inv_sigma2_1, const float *inv_sigma2_2, const float cam1[4], const float cam2[4],
                        const float sim3_in[13], float th2, int fix_scale, double sim3_out[8], uint8_t *bad, int32_t *n_in,
                        orbfe_optsim3_stats *stats, double *chi2_12, double *chi2_21);

/* -------------------------------------------------------------------------- */
/* Optimizer::LocalBundleAdjustment (src/Optimizer.cc:483-814), BundleAdjustment (:54-253) */
/* -------------------------------------------------------------------------- */
/* The bundle adjustment LocalMapping runs per key frame, from :538 on: the caller walks the map graph (:485-536) and hands
 * over the key-frame poses -- the n_local local ones first (optimised unless local_is_fixed[j], i.e. mnId == 0), then the
 * n_fixed ones that only observe local points --, their fx fy cx cy bf, the local points and one edge per observation
 * (u, v = mvKeysUn[idx].pt, u_right = mvuRight[idx] (< 0: a monocular EdgeSE3ProjectXYZ, information inv_sigma2 I2, Huber
 * delta sqrt(5.991); else an EdgeStereoSE3ProjectXYZ, inv_sigma2 I3, sqrt(7.815)), inv_sigma2 = mvInvLevelSigma2[octave]).
 * Edges are grouped by point (edge_point non-decreasing), in the order the reference adds them.  The call runs optimize(5)
 * with the Huber kernels, the first classification (chi2 > 5.991 / 7.815 or depth not positive: level 1; every kernel off),
 * optimize(10) on the level-0 edges and the final classification; g2o's Levenberg loop runs on the host and reads one small
 * record per linearisation and per trial, the passes (linearisation, Schur complement of the points, dense Cholesky of the
 * reduced camera system, back-substitution, errors) are kernels.  Arithmetic is binary64 on inputs widened from float; every
 * sum has a fixed order, so two calls return the same bits.  As in the reference a classification reads the chi2
 * of the last pass the edge was active in -- the last Levenberg trial, accepted or not; for a level-1 edge its round-one
 * value -- while isDepthPositive() is evaluated at the final estimates.
 * Outputs: Tcw_out = SE3Quat::to_homogeneous_matrix of every local pose (a local_is_fixed one: its input through
 * Converter::toSE3Quat); xw_out; erase[e] = 0 kept, 1 in vToErase and level 1 after round one, 2 in vToErase by the final
 * test only (nonzero <=> the reference puts the pair into vToErase; an edge that was level 1 but passes the final test --
 * possible only when its depth turned positive -- is 0); level1[e] (may be NULL) = at level 1 after round one;
 * edge_chi2[e] (may be NULL) what the final test read.  EraseMapPointMatch / EraseObservation, SetPose, SetWorldPos,
 * UpdateNormalAndDepth and the map mutex stay with the caller.
 * stop_flag (may be NULL) is pbStopFlag, polled where the reference polls it: up at entry, the call returns with
 * stats->stopped = 1 and the outputs equal to the converted inputs, erase[] zero; up later, the running optimize() ends
 * and, when up at :698, round two and the first classification are skipped.
 * stats (may be NULL): per round iterations, trials, the final lambda, the robust chi2 of the estimate and why optimize()
 * ended (0 never ran / no active edge, 1 iteration count, 2 ten trials, 3 rho == 0, 4 the nBad >= 3 rule, 5 stop flag).
 * Returns ORBFE_ERR_INVALID before anything is enqueued for: NULL arrays, n_local < 1, more than 256 local key frames, an
 * index out of range, free poses x points above 16777216, edges not grouped by point, a non-finite input, a point or a free pose without any edge, two edges
 * between the same pose and point.  Runs on the calling thread's matcher stream and is complete on return. */
typedef struct orbfe_lba_stats {
  int32_t rounds, stopped, host_syncs, n_level1;
  int32_t iterations[2], trials[2], termination[2];
  double lambda[2], chi2[2];
} orbfe_lba_stats;
int orbfe_local_bundle_adjustment(int device, int n_local, int n_fixed, const float *Tcw /*[n_local+n_fixed,16], local first*/,
                                  const uint8_t *local_is_fixed /*[n_local]; may be NULL*/,
                                  const float *cam /*[n_local+n_fixed,5]: fx fy cx cy bf*/, int n_points, const float *xw /*[n_points,3]*/,
                                  int n_edges, const int32_t *edge_pose, const int32_t *edge_point /*non-decreasing*/,
                                  const float *u, const float *v, const float *u_right /*<0: monocular*/, const float *inv_sigma2,
                                  const volatile int *stop_flag /*may be NULL*/, double *Tcw_out /*[n_local,16]*/,
                                  double *xw_out /*[n_points,3]*/, uint8_t *erase /*[n_edges]*/, uint8_t *level1 /*[n_edges]; may be NULL*/,
                                  orbfe_lba_stats *stats, double *edge_chi2 /*[n_edges]; may be NULL*/);
/* Optimizer::BundleAdjustment (:54-253) on the same operands (every key frame is local, fixed when mnId == 0; fixed ones may
 * still be appended): ONE optimize(n_iterations), Huber kernels when robust != 0, no classification, so there is no
 * erase[].  stop_flag is polled before every iteration and inside the trial loop.  stats->...[1] stay 0. */
int orbfe_bundle_adjustment(int device, int n_local, int n_fixed, const float *Tcw, const uint8_t *local_is_fixed, const float *cam,
                            int n_points, const float *xw, int n_edges, const int32_t *edge_pose, const int32_t *edge_point,
                            const float *u, const float *v, const float *u_right, const float *inv_sigma2, int n_iterations,
                            int robust, const volatile int *stop_flag, double *Tcw_out, double *xw_out, orbfe_lba_stats *stats,
                            double *edge_chi2 /*may be NULL*/);
/* orbfe_local_bundle_adjustment with the points in a resident table: point p is slot[p] (distinct slots); its position is
 * gathered from the table on the device and the optimised position written back to the same slot as a float (SetWorldPos),
 * so only poses, slots, edges and flags travel.  Normal and distance range are the caller's UpdateNormalAndDepth, written
 * through orbfe_mappoints_update.  xw_out may be NULL.  Every output is bit-equal to the array form on the table's floats.
 * When the flag is up at entry the table is left as it is and xw_out is not written.  The table's lock is held for the whole
 * call (every Levenberg trial synchronises with the host), so other calls on the same table wait for it.  Slots named twice
 * are refused. */
int orbfe_local_bundle_adjustment_mappoints(orbfe_mappoints *mp, int n_points, const int32_t *slot, int n_local, int n_fixed,
                                            const float *Tcw, const uint8_t *local_is_fixed, const float *cam, int n_edges,
                                            const int32_t *edge_pose, const int32_t *edge_point, const float *u, const float *v,
                                            const float *u_right, const float *inv_sigma2, const volatile int *stop_flag,
                                            double *Tcw_out, double *xw_out /*may be NULL*/, uint8_t *erase, uint8_t *level1,
                                            orbfe_lba_stats *stats, double *edge_chi2);

/* Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:833-1104) from the graph on: the 7-DoF pose graph over every key frame
 * of the map that LoopClosing::CorrectLoop runs after a loop is closed.  Vertex v is a VertexSim3Expmap with estimate sim3[v]
 * (vScw: CorrectedSim3[pKF] if present, else Sim3(Rcw, tcw, 1); the record of orbfe_optimize_sim3: qx qy qz qw tx ty tz s),
 * fixed when is_fixed[v] (pKF == pLoopKF; NULL: none).  Edge e is an EdgeSim3 with identity information and no robust
 * kernel, vertex 0 = edge_i[e], vertex 1 = edge_j[e]; its measurement Sji = S[j] * S[i]^-1 is computed by the library from
 * sim3_meas (Snc: NonCorrectedSim3[k] if present, else vScw[k]; NULL: the same as sim3) when edge_kind[e] == 0 -- spanning
 * tree, old loop and covisibility edges (:939-1040) -- and from sim3 when edge_kind[e] == 1 -- the new LoopConnections
 * (:907-936); edge_kind NULL: all 0.  Which edges exist, and their de-duplication, is the caller's (two edges between one
 * pair are legal).  Levenberg with lambda_init = 1e-16 and optimize(n_iterations) (20 in the reference): the loop runs on the
 * host and reads one small record per linearisation and per trial; the linearisation (analytic Jacobians), the
 * assembly of the block-sparse normal equations, the block-sparse Cholesky factorisation (7 x 7 blocks, the caller's vertex
 * order, symbolic part on the host) with its substitutions, and the errors are kernels.  Arithmetic is binary64 and every sum
 * has a fixed order, so two calls return the same bits.  A failed factorisation is a zero step and a rejected trial.
 * Outputs: sim3_out[v] the optimised Siw; Tiw_out[v] = [R | t / s] as floats (:1059-1067); edge_chi2 (may be NULL) the chi2
 * of the last evaluation of the edge (the last Levenberg trial, accepted or not).  An edge between two fixed vertices is not
 * active: its edge_chi2 is that of the inputs and it takes no part in stats->chi2.  A free vertex without edges is legal (its
 * step is zero).  With no free vertex, no active edge or n_iterations == 0 nothing is optimised and the outputs are the
 * inputs.  stats (may be NULL): termination as in orbfe_lba_stats; host_syncs = iterations + trials + 1; n_free, blocks_A and
 * blocks_L the free vertices and the blocks of the lower triangle, diagonal included, of H and of its factor; solve_failures
 * the trials whose factorisation met a pivot that was not positive; lambda, chi2_initial and chi2.
 * Returns ORBFE_ERR_INVALID before anything is enqueued for: NULL arrays, an edge with i == j, an edge index out of range,
 * an edge_kind above 1, a non-finite input, a scale <= 0, n_iterations < 0; ORBFE_ERR_CAPACITY when the factor has more than
 * 262144 blocks or the factorisation more than 4194304 block updates.  Runs on the calling thread's matcher stream and is
 * complete on return.  SetPose, SetWorldPos, UpdateNormalAndDepth and the map mutex stay with the caller. */
typedef struct orbfe_essgraph_stats {
  int32_t iterations, trials, termination, stopped, host_syncs;
  int32_t n_free, blocks_A, blocks_L;
  int32_t solve_failures;
  double lambda, chi2_initial, chi2;
} orbfe_essgraph_stats;
int orbfe_optimize_essential_graph(int device, int n_vertices, const double *sim3 /*[n_vertices,8]*/,
                                   const double *sim3_meas /*[n_vertices,8]; may be NULL*/, const uint8_t *is_fixed /*[n_vertices]; may be NULL*/,
                                   int n_edges, const int32_t *edge_i, const int32_t *edge_j, const uint8_t *edge_kind /*may be NULL*/,
                                   int fix_scale, int n_iterations, double *sim3_out /*[n_vertices,8]*/, float *Tiw_out /*[n_vertices,16]*/,
                                   double *edge_chi2 /*[n_edges]; may be NULL*/, orbfe_essgraph_stats *stats);
/* The tail of OptimizeEssentialGraph (:1070-1103): P <- Sout[r]^-1 .map( S[r] .map(P) ) for every point, r = ref_vertex[p] its
 * reference key frame (mnCorrectedReference where mnCorrectedByKF is the current key frame); sim3 is the vScw the
 * optimisation was given, sim3_out what it returned.  In double, stored as float; ref_vertex[p] == -1 copies the point
 * through (a bad map point). */
int orbfe_essential_graph_correct_points(int device, int n_vertices, const double *sim3, const double *sim3_out, int n_points,
                                         const float *xw /*[n_points,3]*/, const int32_t *ref_vertex, float *xw_out /*[n_points,3]*/);
/* The same on a resident table: the positions of slot[0 .. n_slots) (distinct slots) are rewritten in place, bit-equal to the
 * array form.  Normal and distance range are the caller's UpdateNormalAndDepth, written through orbfe_mappoints_update. */
int orbfe_essential_graph_correct_mappoints(orbfe_mappoints *table, int n_vertices, const double *sim3, const double *sim3_out,
                                            int n_slots, const int32_t *slot, const int32_t *ref_vertex);
/* GetWorldPos of slot[0 .. n_slots) as the table holds it: what orbfe_essential_graph_correct_mappoints (or the table form of
 * the local bundle adjustment) left there, for the caller's SetWorldPos. */
int orbfe_mappoints_positions(orbfe_mappoints *table, int n_slots, const int32_t *slot, float *xw_out /*[n_slots,3]*/);
/* GetDescriptor of slot[0 .. n_slots) as the table holds it: what orbfe_mappoints_update or
 * orbfe_obsgraph_distinctive_descriptors_mappoints wrote (a slot that was never written holds zeros). */
int orbfe_mappoints_descriptors(orbfe_mappoints *table, int n_slots, const int32_t *slot, uint8_t *desc_out /*[n_slots,32]*/);
/* The linear solver of orbfe_optimize_essential_graph on its own (diagnostic and test surface; the optimiser uses the very
 * same kernels): A x = rhs for a symmetric positive definite A of 7 x 7 blocks given by its block lower triangle in
 * block-CSC -- column c holds blocks [colptr[c], colptr[c + 1]), the first of them the diagonal block (its lower triangle is
 * read), rows ascending -- blocks[k] row-major.  *ok = 0 and x = 0 when a pivot is not positive; *blocks_L (may be NULL) the
 * blocks of the factor. */
int orbfe_block_sparse_solve7(int device, int n_block_cols, const int32_t *colptr, const int32_t *rowidx, const double *blocks /*[.,49]*/,
                              const double *rhs /*[7 n_block_cols]*/, double *x, int32_t *ok, int32_t *blocks_L);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th,
 * const bool bMono) (src/ORBmatcher.cc:1484-1633) after the caller's pose arithmetic: last-frame
 * point i is valid when it has a non-outlier map point with invzc >= 0 projecting to (u, v) inside
 * the image; last_octave / last_angle are LastFrame.mvKeysUn[i]; mp_desc its map point's
 * descriptor; obs_positive[i] = Observations()>0 (NULL = all).  mode 0: levels
 * [octave-1, octave+1]; 1 (bForward): >= octave; 2 (bBackward): <= octave.  mbf / invzc are read
 * only for frames with u_right.  blocked[i2] != 0 <=> CurrentFrame.mvpMapPoints[i2] holds a point with
 * Observations() > 0 at entry (:1572-1574; NULL = none, which is the state Tracking::TrackWithMotionModel calls it in).
 * match_cur[i2] = last-frame index or -1. */
int orbfe_search_by_projection_last_frame(int device, const orbfe_frame_view *Cur,
                                          const float *scale_factors, int n_levels, float mbf,
                                          int n_last, const uint8_t *valid, const float *u,
                                          const float *v, const float *invzc,
                                          const int32_t *last_octave, const float *last_angle,
                                          const uint8_t *mp_desc, const uint8_t *obs_positive,
                                          const uint8_t *blocked, int mode, float th, int check_orientation,
                                          int32_t *match_cur, int32_t *n_matches);

/* ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const set<MapPoint*> &sAlreadyFound,
 * const float th, const int ORBdist) (src/ORBmatcher.cc:1641-1775, relocalisation) after the caller's
 * projection: point i is valid when pKF's map point i exists, is good, is not in sAlreadyFound,
 * projects to (u, v) inside the image and lies inside its distance range; level = PredictScale;
 * kf_angle = pKF->mvKeysUn[i].angle.  blocked[i2] != 0 <=> CurrentFrame.mvpMapPoints[i2] != NULL
 * (NULL = none). */
int orbfe_search_by_projection_keyframe(int device, const orbfe_frame_view *Cur,
                                        const float *scale_factors, int n_levels,
                                        const uint8_t *blocked, int n, const uint8_t *valid,
                                        const float *u, const float *v, const int32_t *level,
                                        const float *kf_angle, const uint8_t *mp_desc, float th,
                                        int orb_dist, int check_orientation, int32_t *match_cur,
                                        int32_t *n_matches);

/* The same search of ONE current frame against the projected map points of n_candidates key frames in one call
 * (Tracking::Relocalization, src/Tracking.cc:1577,1595: per candidate whose PnP pose survived, th = 10 then 3, ORBdist = 100
 * then 64).  Candidate k brings n[k] points and its own arrays valid[k] / u[k] / v[k] / level[k] / kf_angle[k] / mp_desc[k] /
 * blocked[k] (blocked, or blocked[k], may be NULL), window th[k] and bound orb_dist[k].  One upload of all query lists, one
 * launch group, one download; the frame itself goes up once (or not at all when resident).
 * match_cur [k * Cur->n + i2], n_matches [k]; every output equals the single call. */
int orbfe_search_by_projection_keyframe_multi(int device, const orbfe_frame_view *Cur, const float *scale_factors,
                                              int n_levels, int n_candidates, const uint8_t *const *blocked,
                                              const int32_t *n, const uint8_t *const *valid, const float *const *u,
                                              const float *const *v, const int32_t *const *level,
                                              const float *const *kf_angle, const uint8_t *const *mp_desc,
                                              const float *th, const int32_t *orb_dist, int check_orientation,
                                              int32_t *match_cur, int32_t *n_matches);

/* ORBmatcher::SearchByProjection(KeyFrame *pKF, cv::Mat Scw, const vector<MapPoint*> &vpPoints,
 * vector<MapPoint*> &vpMatched, int th) (src/ORBmatcher.cc:335-449, loop closing) after the caller's
 * Sim3 projection.  matched[idx] != 0 <=> vpMatched[idx] != NULL before the call (NULL = none);
 * match[idx] = point newly matched to keypoint idx or -1. */
int orbfe_search_by_projection_sim3(int device, const orbfe_frame_view *KF, const float *scale_factors,
                                    int n_levels, const uint8_t *matched, int n, const uint8_t *valid,
                                    const float *u, const float *v, const int32_t *level,
                                    const uint8_t *mp_desc, float th, int32_t *match,
                                    int32_t *n_matches);

/* ORBmatcher::SearchForInitialization(Frame &F1, Frame &F2, vector<cv::Point2f> &vbPrevMatched,
 * vector<int> &vnMatches12, int windowSize) (src/ORBmatcher.cc:469-603).  prev_x / prev_y are
 * vbPrevMatched, updated in place like the reference; match12[i1] = i2 or -1. */
int orbfe_search_for_initialization(int device, const orbfe_frame_view *F1, const orbfe_frame_view *F2,
                                    float *prev_x, float *prev_y, int window_size, float nnratio,
                                    int check_orientation, int32_t *match12, int32_t *n_matches);

/* Diagnostics: the projection searches above replay the reference's order-dependent claim loops on the device as a
 * fixed-point iteration (csrc/k_window.hip: k_window_claim); this is the largest number of rounds a claim job of the calling
 * thread's LAST such call took (1 + the longest chain of points that depend on each other; 2-3 on real frames). */
int orbfe_debug_last_claim_rounds(void);

/* The search ORBmatcher::Fuse runs per map point (src/ORBmatcher.cc:940-1110 with chi2_gate != 0,
 * the Sim3 overload :1112-1249 with chi2_gate == 0): best_idx[i] = keypoint of pKF with octave in
 * [level-1, level], passing the reprojection gate (5.99 mono / 7.8 stereo on e2 *
 * inv_level_sigma2[octave]) and the least descriptor distance <= TH_LOW, or -1.  What happens to a hit
 * (Replace / AddObservation) is map bookkeeping and stays with the caller. */
int orbfe_fuse_search(int device, const orbfe_frame_view *KF, const float *scale_factors,
                      const float *inv_level_sigma2, int n_levels, int n, const uint8_t *valid,
                      const float *u, const float *v, const float *ur, const int32_t *level,
                      const uint8_t *mp_desc, float th, int chi2_gate, int32_t *best_idx);

/* ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1251-1482) after the caller's two projections:
 * valid1[i1] <=> keypoint i1 of KF1 has a good map point, not matched yet, that projects into KF2 at
 * (u1, v1) inside the image and its distance range, level1 = PredictScale, desc1 = its descriptor;
 * the "2" arrays are the KF2 -> KF1 direction.  match12[i1] = i2 for mutually consistent pairs. */
int orbfe_search_by_sim3(int device, const orbfe_frame_view *KF1, const orbfe_frame_view *KF2,
                         const float *scale_factors1, const float *scale_factors2, int n_levels,
                         const uint8_t *valid1, const float *u1, const float *v1, const int32_t *level1,
                         const uint8_t *desc1, const uint8_t *valid2, const float *u2, const float *v2,
                         const int32_t *level2, const uint8_t *desc2, float th, int32_t *match12,
                         int32_t *n_found);

/* cv::initUndistortRectifyMap(K, D, R, P.rowRange(0,3).colRange(0,3), cv::Size(cols, rows), CV_32F, M1, M2) as
 * Examples/Stereo/stereo_euroc.cc:97-98 calls it once at start-up: the two CV_32F maps orbfe_rectifier_create takes, from the
 * calibration of the settings file (Examples/Stereo/EuRoC.yaml: LEFT.K / LEFT.D / LEFT.R / LEFT.P).  K, R, P: row-major 3 x 3
 * doubles (R NULL = identity, P NULL = K; pass the first three columns of a 3 x 4 projection); D: n_dist = 0, 4, 5 or 8
 * coefficients (k1 k2 p1 p2 [k3 [k4 k5 k6]]); map_x / map_y: width * height floats each, written on the host.  Evaluated on the
 * device, one thread per map row (a row is the reference's sequential running-sum chain in double precision). */
int orbfe_init_undistort_rectify_map(int device, const double *K, const double *D, int n_dist, const double *R,
                                     const double *P, int width, int height, float *map_x, float *map_y);

/* cv::remap(im, imRect, M1, M2, cv::INTER_LINEAR) with CV_32F maps and the default constant-0
 * border, 8-bit single channel: the EuRoC rectification of Examples/Stereo/stereo_euroc.cc:136-137
 * (the maps come from cv::initUndistortRectifyMap at :97-98, once, and are handed over here once).
 * Destination size = map size (width x height, map_stride floats per row). */
typedef struct orbfe_rectifier orbfe_rectifier;
int orbfe_rectifier_create(int device, const float *map_x, const float *map_y, int width, int height,
                       int map_stride, orbfe_rectifier **out);
void orbfe_rectifier_destroy(orbfe_rectifier *r);
/* Host buffers, one frame. */
int orbfe_remap(orbfe_rectifier *r, const uint8_t *src, int src_width, int src_height, int src_stride,
                uint8_t *dst, int dst_stride);
/* Device-resident frames: rectified images are written where orbfe_extract_batch_device reads them.
 * Enqueued on the default stream, complete on return (see orbfe_cvt_gray_batch_device). */
int orbfe_remap_batch_device(orbfe_rectifier *r, const uint8_t *d_src, int n_frames, int src_width,
                             int src_height, int src_stride, size_t src_frame_stride, uint8_t *d_dst,
                             int dst_stride, size_t dst_frame_stride);

/* The stereo front end of Examples/Stereo/stereo_euroc.cc for a device-resident batch of RAW pairs: cv::remap of the
 * left and of the right image (:136-137) and the two ExtractORB calls of the stereo Frame constructor
 * (src/Frame.cc:78-81), enqueued sub-batch by sub-batch on extractor e's streams (returns at once, like
 * orbfe_extract_batch_device_async; no host wait between rectification and extraction).  Raw frame p of either eye at
 * d_raw_*[p*src_frame_stride ..]; rectified frames are written tightly packed and interleaved to d_rectified
 * (2*n_pairs frames of width x height of the rectifiers: L0, R0, L1, R1, ...), which is also where the extractor's
 * level 0 -- and orbfe_stereo_match_batch_device's SAD windows -- are read from, so it must stay valid until the
 * matchers of this batch are done.  Outputs as orbfe_extract_batch_device for 2*n_pairs frames. */
int orbfe_extract_stereo_rectified_batch_device_async(
    orbfe_extractor *e, orbfe_rectifier *rect_left, orbfe_rectifier *rect_right, const uint8_t *d_raw_left,
    const uint8_t *d_raw_right, int n_pairs, int src_width, int src_height, int src_stride, size_t src_frame_stride,
    uint8_t *d_rectified, orbfe_keypoint *d_keypoints, uint8_t *d_descriptors, int capacity, int32_t *d_n_out);

/* cv::undistortPoints(mat, mat, mK, mDistCoef, cv::Mat(), mK) as Frame::UndistortKeyPoints and
 * Frame::ComputeImageBounds call it (src/Frame.cc:443-475, 481-510).  K4 = fx, fy, cx, cy (the
 * CV_32F entries of mK); dist = k1, k2, p1, p2[, k3[, k4, k5, k6]] (n_dist 0, 4, 5 or 8); xy /
 * out_xy are n (x, y) float pairs. */
int orbfe_undistort_points(int device, const float *xy, int n, const float *K4, const float *dist,
                           int n_dist, float *out_xy);
/* mvKeysUn of a device-resident extractor batch (the layout orbfe_extract_batch_device writes):
 * records copied, pt undistorted.  Enqueued on the default stream, complete on return (see
 * orbfe_cvt_gray_batch_device). */
int orbfe_undistort_keypoints_batch_device(int device, const orbfe_keypoint *d_keypoints,
                                           const int32_t *d_n, int n_frames, int capacity,
                                           const float *K4, const float *dist, int n_dist,
                                           orbfe_keypoint *d_keypoints_un);
/* Frame::ComputeImageBounds (src/Frame.cc:481-510): bounds4 = mnMinX, mnMaxX, mnMinY, mnMaxY. */
int orbfe_compute_image_bounds(int device, int cols, int rows, const float *K4, const float *dist,
                               int n_dist, float *bounds4);
/* Frame::ComputeStereoFromRGBD (src/Frame.cc:689-713): kx / ky = mvKeys[i].pt, kux = mvKeysUn[i].pt.x,
 * depth_image = imDepth (CV_32F, after the mDepthMapFactor scaling of src/Tracking.cc:226-227). */
int orbfe_stereo_from_rgbd(int device, const float *kx, const float *ky, const float *kux, int n,
                           const float *depth_image, int width, int height, int stride_floats,
                           float mbf, float *u_right, float *depth);

/* ------------------------------------------------------------------------- */
/* Observation graph: MapPoint::mObservations resident on the device, and the */
/* four loops over it (covisibility votes, key-frame culling, normal / depth)  */
/* ------------------------------------------------------------------------- */
/* The table map point -> the key frames that see it, indexed by point SLOT (the slot space of an orbfe_mappoints table:
 * one slot list serves both) and by KF SLOT (the caller keeps the KeyFrame* <-> kf slot map and gives each key frame
 * its mnId).  One row of row_width entries per point slot (a power of two in 8 .. 256, fixed at create; an entry is the
 * 8-byte orbfe_observation), and per point slot the live entry count, nObs (a stereo observation weighs 2, as
 * MapPoint::AddObservation / EraseObservation count, src/MapPoint.cc:101-145), a bad flag and the kf slot of mpRefKF;
 * per kf slot mnId, the camera centre Ow and a bad flag.  A slot that was never set counts as bad.
 *
 * Deviation (row order): the reference iterates std::map<KeyFrame*, size_t> in POINTER order, which differs from run
 * to run.  This table keeps every row in ascending mnId of the observing key frame -- one of the orders the reference
 * can take, and the one every result below is defined by.  It matters for the float sum of update_normal_depth and for
 * which key frame becomes the reference after an erase ("mObservations.begin()": here the lowest remaining mnId).
 *
 * The host keeps a mirror of everything; the mutations below change the mirror alone -- they need no device and touch
 * none -- and mark the rows they changed.  A call that reads the table on the device (votes, culling_counts,
 * update_normal_depth*, get_row from the device) first rewrites the marked rows, each as a whole (at most 2 KB), then
 * runs on the handle's one stream and is complete on return.  Every operand is checked on the host before anything is
 * enqueued: slots out of range, NULL arrays and n < 0 return ORBFE_ERR_INVALID.  A handle serialises its own calls;
 * creating one does not touch the device.  Without a device the reading calls return ORBFE_ERR_HIP: no CPU fallback.
 * Limits: point_capacity <= 2^24, kf_capacity <= 2^20, point_capacity * row_width <= 2^28. */
typedef struct orbfe_obsgraph orbfe_obsgraph;
typedef struct orbfe_observation {
  int32_t kf_slot;
  uint16_t idx;   /* mObservations[pKF] */
  uint8_t octave; /* pKF->mvKeysUn[idx].octave */
  uint8_t flags;  /* bit 0: pKF->mvuRight[idx] >= 0 */
} orbfe_observation;

int orbfe_obsgraph_create(int device, int point_capacity, int kf_capacity, int row_width, orbfe_obsgraph **out);
void orbfe_obsgraph_destroy(orbfe_obsgraph *g);
/* Back to the state after create (the device memory stays with the handle). */
int orbfe_obsgraph_clear(orbfe_obsgraph *g);
/* kf_slot[i] holds key frame kf_id[i] (mnId >= 0) with camera centre Ow[3 i ..] (GetCameraCenter()) and isBad() = bad[i].
 * Two kf slots never hold one id, and the id of a kf slot that rows still name cannot change (the rows are ordered by
 * it): both return ORBFE_ERR_INVALID with nothing applied. */
int orbfe_obsgraph_set_keyframes(orbfe_obsgraph *g, int n, const int32_t *kf_slot, const int64_t *kf_id, const float *Ow,
                                 const uint8_t *bad);
/* isBad() and mpRefKF (a kf slot, -1 = none) of n point slots.  The rows stay as they are: the kernels skip a bad point. */
int orbfe_obsgraph_set_points(orbfe_obsgraph *g, int n, const int32_t *slot, const uint8_t *bad, const int32_t *ref_kf_slot);
/* MapPoint::AddObservation(pKF, idx) (:101-114) n times, in order: a (slot, kf_slot) pair already present is ignored, as
 * the count(pKF) early return does; nObs += stereo[i] ? 2 : 1.  The kf slot must have been set.  A full row returns
 * ORBFE_ERR_CAPACITY with NOTHING of the call applied. */
int orbfe_obsgraph_add_observations(orbfe_obsgraph *g, int n, const int32_t *slot, const int32_t *kf_slot, const uint16_t *idx,
                                    const uint8_t *octave, const uint8_t *stereo);
/* MapPoint::EraseObservation(pKF) (:119-145) n times, in order: an absent pair is ignored; nObs drops by 1 or 2; if the
 * erased key frame was the reference, the reference moves to the row's first remaining entry; nObs <= 2 marks the point
 * bad and clears its row (SetBadFlag, :164-182; nObs keeps its value) -- became_bad[i] = 1 (may be NULL).  Deviation: the
 * reference of a row that empties becomes -1 (the reference dereferences begin() of an empty map). */
int orbfe_obsgraph_erase_observations(orbfe_obsgraph *g, int n, const int32_t *slot, const int32_t *kf_slot, uint8_t *became_bad);
/* The map-point part of KeyFrame::SetBadFlag (src/KeyFrame.cc:488 ff.): EraseObservation(kf) on every point that lists
 * the key frame, the key frame marked bad; out_slots = the points that became bad, ascending, *n_out of them.  More than
 * `capacity` returns ORBFE_ERR_CAPACITY with *n_out set and nothing applied.  The covisibility edges and the spanning
 * tree stay with the caller. */
int orbfe_obsgraph_erase_keyframe(orbfe_obsgraph *g, int kf_slot, int32_t *out_slots, int capacity, int *n_out);
/* Test read-back of one point slot: from the host mirror (from_device = 0; needs no device) or from the device table
 * (from_device != 0, after the pending rows were written).  entries holds row_width records, the live ones first, the
 * rest zero. */
int orbfe_obsgraph_get_row(orbfe_obsgraph *g, int from_device, int slot, orbfe_observation *entries, int32_t *n_entries,
                           int32_t *n_obs, uint8_t *bad, int32_t *ref_kf_slot);

/* The counting loop of KeyFrame::UpdateConnections (src/KeyFrame.cc:326-344) and of Tracking::UpdateLocalKeyFrames
 * (src/Tracking.cc:1346-1362) for n_queries point lists in one launch: query q is q_slots [q_offsets[q], q_offsets[q+1])
 * -- a key frame's (a frame's) non-NULL mvpMapPoints.  Bad points are skipped; every entry of every other point's row
 * adds 1 to its key frame's counter, except entries of self_kf_slot[q] (-1: none; the mnId == mnId test of :340).  A slot
 * named twice votes twice.  Per query: the kf slots with a non-zero counter in ASCENDING KF-SLOT order and their
 * counters, [q * capacity ..], count[q] of them; equal inputs give equal arrays.  A count above `capacity` fills
 * `capacity` entries and returns ORBFE_ERR_CAPACITY (every count[] is still set).  At most 65535 queries per call.
 * The counters are int32 in the workgroup's LDS for kf_capacity <= 8192, above that in a workspace of
 * n_queries * kf_capacity int32. */
int orbfe_obsgraph_votes(orbfe_obsgraph *g, int n_queries, const int32_t *q_offsets, const int32_t *q_slots,
                         const int32_t *self_kf_slot, int capacity, int32_t *kf_slot_out, int32_t *weight_out, int32_t *count);
/* The counting of LocalMapping::KeyFrameCulling (src/LocalMapping.cc:729-769) for n_kf candidates in one launch.
 * Candidate c is kf_slot[c]; its features slot / octave [offsets[c], offsets[c+1]) are the ones that pass the host-side
 * tests of :732-740 (a map point, and for stereo / RGB-D 0 <= mvDepth <= mThDepth), each with mvKeysUn[i].octave.  Per
 * listed feature: a bad point is skipped; n_mps[c]++; if nObs > 3, the row's entries with kf_slot != kf_slot[c] and
 * octave_i <= octave + 1 are counted, and 3 or more give n_redundant[c]++ (the reference's early break does not change
 * ">= 3").  The counts describe the table as it stands at entry; the caller culls when n_redundant > 0.9 * n_mps. */
int orbfe_obsgraph_culling_counts(orbfe_obsgraph *g, int n_kf, const int32_t *kf_slot, const int32_t *offsets, const int32_t *slot,
                                  const uint8_t *octave, int32_t *n_mps, int32_t *n_redundant);
/* MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:360-404) for n point slots at the positions pos[3 i ..]
 * (scale_factors = mvScaleFactors, n_levels = mnScaleLevels, 1 .. 256).  A restatement of :378-402 as OpenCV's
 * Mat / double and Mat + MatExpr evaluate them, in IEEE binary32 with no contraction, over the row left to right
 * (ascending mnId); it equals the reference up to the observer order and the last place:
 *   per entry k: d = P - Ow_k (per component); nrm = sqrt(sum (double)d_i^2); a = (float)(1.0 / nrm);
 *                normal_i = normal_i + d_i * a;
 *   at the end:  normal_i = normal_i * (float)(1.0 / n), n = the row's entry count;
 *   PC = P - Ow_ref; dist = (float)sqrt(sum (double)PC_i^2); max_dist = dist * scale_factors[level], level = the octave of
 *   the reference key frame's entry; min_dist = max_dist / scale_factors[n_levels - 1].
 * The sum over a row is sequential by definition: lanes compute the terms, one chain adds them in row order.
 * valid[i] = 0 -- and normal / min_dist / max_dist [i] are NOT written -- for a bad point, an empty row, and a reference
 * key frame that is not in the row (deviation: the reference's observations[pRefKF] would silently insert index 0).  A
 * reference entry whose octave is not below n_levels returns ORBFE_ERR_INVALID before anything is enqueued. */
int orbfe_obsgraph_update_normal_depth(orbfe_obsgraph *g, int n, const int32_t *slot, const float *pos, const float *scale_factors,
                                       int n_levels, float *normal, float *min_dist, float *max_dist, uint8_t *valid);
/* The same on a resident map-point table: pos is read from mp's slot and normal / min_dist / max_dist are written into
 * it, bit-equal to the array form; only the slot list travels.  Slots with valid = 0 keep what they hold.  Both handles
 * must be on one device and g's point_capacity must not exceed mp's capacity, and no slot may be named twice
 * (ORBFE_ERR_INVALID).  Takes g's serialisation, then mp's. */
int orbfe_obsgraph_update_normal_depth_mappoints(orbfe_obsgraph *g, orbfe_mappoints *mp, int n, const int32_t *slot,
                                                 const float *scale_factors, int n_levels, uint8_t *valid);

/* KeyFrame::UpdateConnections :347-393 over ONE query's votes, KFcounter = (kf_id, weight)[n] (mnIds, any order, weights
 * positive).  th = 15; when nobody reaches it the maximum alone is connected.  ordered_id / ordered_weight:
 * mvpOrderedConnectedKeyFrames / mvOrderedWeights; connect_id / connect_weight: who receives AddConnection(this, weight),
 * in ascending id; *parent_id: mvpOrderedConnectedKeyFrames.front() (for mbFirstConnection; -1 when n = 0, where the
 * reference returns early and every count is 0).  mConnectedKeyFrameWeights is the input itself.  Every output array
 * holds n entries.  Deviation: ties break by mnId where the reference breaks them by pointer -- sort() of
 * pair<int, KeyFrame*> ascends, so after push_front equal weights come out in DESCENDING id, and the strict > of the nmax
 * scan keeps the LOWEST id.  Host code: needs no device. */
int orbfe_obsgraph_update_connections(int n, const int64_t *kf_id, const int32_t *weight, int64_t *ordered_id,
                                      int32_t *ordered_weight, int *n_ordered, int64_t *connect_id, int32_t *connect_weight,
                                      int *n_connect, int64_t *parent_id);
/* Tracking::UpdateLocalKeyFrames :1364-1454 over ONE frame's votes, keyframeCounter = (kf_id, weight, bad = isBad())[n].
 * K1: the voted key frames in ascending id, bad ones skipped, pKFmax under strict >.  K2: for each K1 key frame, in
 * order, the first eligible (not bad, not yet local) of its best 10 covisibles, the first eligible child, and its
 * parent when not yet local -- the reference's break after a parent is added leaves the WHOLE loop, and the loop stops
 * once more than 80 key frames are local.  The loop's end iterator is taken before anything is appended, so it visits
 * the K1 entries while the vector grows.  Record i carries what the walk reads of key frame i:
 * GetBestCovisibilityKeyFrames as neigh_ids / neigh_bad [neigh_offsets[i], neigh_offsets[i+1]) (a longer list may be
 * given: 10 are read), GetChilds() likewise (give them in ascending id), GetParent() as parent_id[i] (-1: none).
 * out_ids: mvpLocalKeyFrames, *n_out of them (more than `capacity`: ORBFE_ERR_CAPACITY, *n_out set); *ref_id: pKFmax
 * (-1: none, mpReferenceKF unchanged).  Host code: needs no device. */
int orbfe_obsgraph_local_keyframes(int n, const int64_t *kf_id, const int32_t *weight, const uint8_t *bad,
                                   const int32_t *neigh_offsets, const int64_t *neigh_ids, const uint8_t *neigh_bad,
                                   const int32_t *child_offsets, const int64_t *child_ids, const uint8_t *child_bad,
                                   const int64_t *parent_id, int64_t *out_ids, int capacity, int *n_out, int64_t *ref_id);

/* ---- The opposite direction: KeyFrame::mvpMapPoints, key frame -> its points, in the same handle ----
 * One row of kf_row_width point slots per kf slot, entry idx = mvpMapPoints[idx] (-1: NULL), with the row's length N.
 * The discipline is the one above: the host mirror is the truth, the three mutations change the mirror alone and mark
 * the rows they touched, the device rows live in a slab of their own that is taken at the first device call after
 * enable, and a reading call (keyframe_points_union, tracked_points, get_keyframe_points from the device) first rewrites
 * the marked rows, each as a whole.  A handle that never calls enable behaves as before and allocates nothing more.
 * Every function below except enable returns ORBFE_ERR_INVALID on a handle that is not enabled.
 * orbfe_obsgraph_clear also empties these rows and keeps the width.  orbfe_obsgraph_erase_keyframe leaves the erased key
 * frame's row as it is: KeyFrame::SetBadFlag (src/KeyFrame.cc:488 ff.) does not clear mvpMapPoints either. */

/* Gives the handle rows of kf_row_width entries: a multiple of 64 in 64 .. 16384 (at least the largest N), with
 * kf_capacity * kf_row_width <= 2^28.  Once per handle: a second call with the same width is a no-op, with another width
 * ORBFE_ERR_INVALID.  Does not touch the device. */
int orbfe_obsgraph_enable_keyframe_points(orbfe_obsgraph *g, int kf_row_width);
/* The whole mvpMapPoints of the key frame in kf_slot, as the KeyFrame constructor copies it from the Frame
 * (src/KeyFrame.cc:42): n = N <= kf_row_width entries, slot[i] in [-1, point_capacity).  The kf slot must have been
 * given to set_keyframes.  The row's length becomes n. */
int orbfe_obsgraph_set_keyframe_points(orbfe_obsgraph *g, int kf_slot, int n, const int32_t *slot);
/* KeyFrame::AddMapPoint(pMP, idx) and ReplaceMapPointMatch(idx, pMP) (src/KeyFrame.cc:220-224, 240-243: both are
 * mvpMapPoints[idx] = pMP) and EraseMapPointMatch(idx) (:226-230; slot[i] = -1), n assignments applied in order.  idx[i]
 * must be below the length of row kf_slot[i] (so a row that was never set takes none).  The call applies as a whole or,
 * with ORBFE_ERR_INVALID, not at all.  EraseMapPointMatch(pMP) (:232-237) is the caller's GetIndexInKeyFrame, then this. */
int orbfe_obsgraph_assign_keyframe_points(orbfe_obsgraph *g, int n, const int32_t *kf_slot, const uint16_t *idx, const int32_t *slot);
/* Test read-back of one row: from the host mirror (from_device = 0; needs no device) or from the device (from_device != 0,
 * after the marked rows were written).  slots holds kf_row_width entries, the row's *n first, the rest -1. */
int orbfe_obsgraph_get_keyframe_points(orbfe_obsgraph *g, int from_device, int kf_slot, int32_t *slots, int32_t *n);
/* The ordered union of key frames' map points, for n_queries key-frame lists in one call: Tracking::UpdateLocalPoints
 * (src/Tracking.cc:1315-1333; query = mvpLocalKeyFrames), and the same loop of LocalMapping::SearchInNeighbors
 * (src/LocalMapping.cc:552-571; vpTargetKFs -> vpFuseCandidates), LoopClosing::ComputeSim3 (src/LoopClosing.cc:417-436;
 * vpLoopConnectedKFs -> mvpLoopMapPoints) and lLocalMapPoints of Optimizer::LocalBundleAdjustment.  Query q is the kf slots
 * q_kf_slots [q_offsets[q], q_offsets[q+1]) in the caller's order.  The key frames are visited in list order and the
 * entries of a row in idx order; -1 is skipped, a point whose record is bad or was never set (set_points) is skipped, a
 * point already emitted for this query is skipped, the others are emitted: slot_out [q * capacity ..] holds the point
 * slots in exactly that order, count[q] of them -- unchanged the slot[] argument of orbfe_search_local_points.  A kf
 * slot named twice contributes nothing the second time; a key frame's own bad flag is not read (none of the four loops
 * reads it).  Equal inputs give equal arrays: the order is fixed by position k * kf_row_width + idx (k: the key frame's
 * place in the query), never by arrival.  A count above `capacity` fills `capacity` entries and returns
 * ORBFE_ERR_CAPACITY (every count[] is still set).  ORBFE_ERR_INVALID: a kf slot out of range or never set, more than
 * 65535 queries, offsets that do not start at 0 or descend, a query with key frames * kf_row_width >= 2^31.  The
 * workspace is point_capacity int32 per query, at most 2^26 int32 at a time: more queries run in several groups. */
int orbfe_obsgraph_keyframe_points_union(orbfe_obsgraph *g, int n_queries, const int32_t *q_offsets, const int32_t *q_kf_slots,
                                         int capacity, int32_t *slot_out, int32_t *count);
/* KeyFrame::TrackedMapPoints(minObs) (src/KeyFrame.cc:264-289) for n_kf key frames in one launch: count[i] = the entries
 * of row kf_slot[i] that are not NULL and not bad and, when min_obs > 0, have nObs >= min_obs (nObs as the point's record
 * holds it: a stereo observation weighs 2).  A kf slot out of range or never set returns ORBFE_ERR_INVALID. */
int orbfe_obsgraph_tracked_points(orbfe_obsgraph *g, int n_kf, const int32_t *kf_slot, int min_obs, int32_t *count);

/* ---- KeyFrame::mDescriptors in the same handle, and MapPoint::ComputeDistinctiveDescriptors over the rows ----
 * With the key frames' descriptors next to the rows, the second call LocalMapping makes on every map point a new key
 * frame touched (src/MapPoint.cc:269-333) needs only a slot list, as update_normal_depth_mappoints does for the first:
 * no walk over mObservations, no descriptor list, no index read back.  The store is independent of
 * enable_keyframe_points.  A handle that never enables it allocates nothing and behaves as before; every function below
 * except enable returns ORBFE_ERR_INVALID on such a handle.
 *
 * A key frame's descriptors never change in the reference, so -- unlike everything else in the handle -- the host keeps
 * NO mirror of the bytes, only the number of rows each kf slot received (0: never set).  The two set calls therefore are
 * the handle's only mutations that TOUCH THE DEVICE: they copy into the store on the handle's stream, are complete on
 * return, and without a device return ORBFE_ERR_HIP.  orbfe_obsgraph_clear resets every count to 0 and keeps the device
 * memory; orbfe_obsgraph_erase_keyframe leaves the descriptors in place (a bad key frame is skipped by its flag). */

/* Gives the handle a store of kf_desc_width descriptors per kf slot: a multiple of 64 in 64 .. 16384 (at least the largest
 * N), with kf_capacity * kf_desc_width <= 2^26 (2 GiB).  Once per handle: the same width again is a no-op, another width
 * ORBFE_ERR_INVALID.  Does not touch the device: uint8 [kf_capacity][kf_desc_width][32] is taken at the first set. */
int orbfe_obsgraph_enable_keyframe_descriptors(orbfe_obsgraph *g, int kf_desc_width);
/* mDescriptors of the key frame in kf_slot: n <= kf_desc_width rows of 32 bytes from the host.  The kf slot must have
 * been given to set_keyframes. */
int orbfe_obsgraph_set_keyframe_descriptors(orbfe_obsgraph *g, int kf_slot, int n, const uint8_t *desc /*[n,32]*/);
/* The same, device to device, from a resident frame's descriptors (all f's features): the copy runs on the handle's
 * stream, ordered behind the frame's build.  The frame must be on the handle's device and may be released after the
 * call. */
int orbfe_obsgraph_set_keyframe_descriptors_frame(orbfe_obsgraph *g, int kf_slot, const orbfe_frame *f);
/* Test read-back from the device: the *n_out rows the kf slot holds into desc_out (room for kf_desc_width rows). */
int orbfe_obsgraph_get_keyframe_descriptors(orbfe_obsgraph *g, int kf_slot, uint8_t *desc_out, int32_t *n_out);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) for n point slots in one call.  Per listed slot:
 *   valid[i] = 0 -- and NOTHING else of entry i is written -- for a bad or never-set point (mbBad, :278), an empty row
 *   (:283), and a row of which no entry remains once the entries of bad key frames are skipped (:292, :296);
 *   the row is read left to right, in ascending mnId (the handle's order; the reference's is pointer order), the
 *   entries whose key frame has the bad flag are skipped (:292); N entries remain, descriptor i = the row idx_i of key
 *   frame kf_i's descriptors;
 *   d[i][j] = the 256-bit Hamming distance (:303-312); the median of row i is the (size_t)(0.5 * (N - 1))-th smallest of
 *   its N distances, the self-distance 0 included (:319-321); the winner is the first i under strict < (:323);
 *   best_kf_slot[i] / best_idx[i] = the winner's entry, desc[32 i ..] = its 32 bytes (:332; desc may be NULL).
 * Integers only: equal inputs give equal bytes.  Checked on the host, from the mirror, before anything is enqueued
 * (ORBFE_ERR_INVALID): the store is not enabled; a slot out of range; a listed point that is not bad has an entry whose
 * key frame received no descriptors, or whose idx is not below that key frame's row count -- whether or not that key
 * frame is bad.  One wave per point; rows of more than 64 entries run with four descriptors per lane. */
int orbfe_obsgraph_distinctive_descriptors(orbfe_obsgraph *g, int n, const int32_t *slot, int32_t *best_kf_slot, int32_t *best_idx,
                                           uint8_t *desc /*[n,32], may be NULL*/, uint8_t *valid);
/* The same on a resident map-point table: the winner's 32 bytes are written into mp's descriptor of the slot and nothing
 * else of the slot changes; slots with valid = 0 keep what they hold.  Only the slot list travels.  Both handles must be
 * on one device, g's point_capacity must not exceed mp's capacity, and no slot may be named twice (ORBFE_ERR_INVALID).
 * After a call that returns ORBFE_ERR_INVALID the table is unchanged.  Takes g's serialisation, then mp's. */
int orbfe_obsgraph_distinctive_descriptors_mappoints(orbfe_obsgraph *g, orbfe_mappoints *mp, int n, const int32_t *slot,
                                                     int32_t *best_kf_slot /*may be NULL*/, int32_t *best_idx /*may be NULL*/,
                                                     uint8_t *valid);

/* ------------------------------------------------------------------------- */
/* ORBmatcher::Fuse on the resident map points                                 */
/* ------------------------------------------------------------------------- */
/* The prologue of ORBmatcher::Fuse(pKF, vpMapPoints, th) (src/ORBmatcher.cc:960-1006; the Sim3 overload :1135-1184 with the
 * caller's decomposition of Scw in pose[k]) for the n map points in slot[] against n_keyframes (<= 64) key-frame poses, as ONE
 * kernel launch.  pose[k] holds what Fuse reads of key frame k: GetRotation / GetTranslation / GetCameraCenter, fx fy cx cy mbf,
 * mnMinX .. mnMaxY, mfLogScaleFactor, mnScaleLevels.  Outputs are [k*n + i]; any may be NULL.  valid[k*n+i] = the point passes
 * every test for key frame k; where it is set, u / v / ur / level / dist are the projection, u - mbf/z, PredictScale and
 * dist3D; elsewhere they are 0.  IEEE binary32 (binary64 where stated), no contraction, sums left to right, in this order:
 *   reject flags & ORBFE_MP_BAD; reject skip[k*n+i] (NULL = none); with a graph, reject a point whose observation row names
 *   kf_slot[k] among its live entries (MapPoint::IsInKeyFrame, :965; a slot at or past g's point_capacity has no row);
 *   xc = ((R00*X + R01*Y) + R02*Z) + t0 (yc, zc likewise); reject zc < 0; invz = 1/zc; x = xc*invz; y = yc*invz;
 *   u = fx*x + cx; v = fy*y + cy (NOT isInFrustum's (fx*xc)*invz; the Sim3 overload's 1.0/z in double, rounded to float, is the
 *   same float quotient: 53 >= 2*24 + 2);
 *   KeyFrame::IsInImage (src/KeyFrame.cc:653-656): reject unless u >= min_x && u < max_x && v >= min_y && v < max_y -- the
 *   upper bounds are strict, unlike isInFrustum's;
 *   ur = u - mbf*invz; PO = P - Ow; dist = (float)sqrt(sum (double)PO_i^2); reject dist < 0.8f*min || dist > 1.2f*max;
 *   reject sum (double)PO_i*(double)Pn_i < 0.5 * (double)dist (a compare in double, nothing is divided, :1000);
 *   level = clamp(ceil(log((double)(max/dist)) / (double)log_scale_factor), 0, n_levels-1).
 * Only the slot list, the mask, the poses and kf_slot[] go up.  Slots outside the table, kf slots outside the graph,
 * n_keyframes > 64, a pose whose n_levels is not 1 .. 64, NULL slot / pose / kf_slot (with g) arrays and handles on
 * different devices return ORBFE_ERR_INVALID before anything is enqueued; n == 0 or n_keyframes == 0 is ORBFE_OK with
 * nothing touched.  Takes g's serialisation, then mp's. */
int orbfe_project_fuse(orbfe_mappoints *mp, orbfe_obsgraph *g /* NULL: no IsInKeyFrame test */, int n, const int32_t *slot,
                       int n_keyframes, const int32_t *kf_slot /* [K], read only with g */,
                       const orbfe_camera_pose *pose /* [K] */, const uint8_t *skip /* [K*n] or NULL */,
                       uint8_t *valid, float *u, float *v, float *ur, int32_t *level, float *dist);

/* ORBmatcher::Fuse (chi2_gate != 0: src/ORBmatcher.cc:940-1099; == 0: the Sim3 overload :1112-1237 with the caller's
 * decomposition of Scw in pose[k]) for the SAME slots against K key frames as ONE call: the projection above writes the
 * query windows (centre (u, v), radius th * scale_factors[level], octaves [level-1, level], ur for the chi-square gate of
 * :1030-1054; without the gate ur is not read, :1197-1214) where the window search reads them, the points' descriptors are
 * gathered from the table once for all K key frames, and the one window-search launch of orbfe_fuse_search_multi runs
 * behind it.  One upload (slot list, mask, poses, kf_slot, level tables), one download.  best_idx[k*n+i] = the keypoint of
 * KF[k] Fuse would take for point i (bestDist <= TH_LOW) or -1; projected[k*n+i] (optional) = the point passed the prologue.
 * best_idx equals orbfe_fuse_search_multi fed with orbfe_project_fuse's outputs and the table's descriptors, bit for bit.
 * Beyond orbfe_project_fuse's checks: pose[k].n_levels > n_levels, NULL KF / scale_factors / best_idx (inv_level_sigma2 when
 * gated), a bad key-frame view and -- gated -- a keypoint octave outside the pyramid return ORBFE_ERR_INVALID before
 * anything is enqueued.
 * What stays with the caller: Replace / AddObservation / AddMapPoint (:1069-1090), the pMPinKF comparison of observation
 * counts, and the Sim3 overload's vpReplacePoint.  Results are computed against the state AT ENTRY: a caller that replays
 * the key frames in order ignores the hits of a point that an earlier key frame's replay made bad, and the hits of a point
 * that the replay placed in that key frame.  One thing the multi form cannot reproduce: MapPoint::Replace ends in
 * ComputeDistinctiveDescriptors, so a survivor's descriptor may change between two key frames of the reference's loop.  A
 * caller who needs that exact sequence calls with K = 1 per key frame and refreshes the table in between with
 * orbfe_obsgraph_distinctive_descriptors_mappoints (orbfe_fuse_search_multi has the same property). */
int orbfe_fuse_mappoints(orbfe_mappoints *mp, orbfe_obsgraph *g, int n, const int32_t *slot, int n_keyframes,
                         const orbfe_frame_view *const *KF, const int32_t *kf_slot, const orbfe_camera_pose *pose,
                         const uint8_t *skip, const float *scale_factors, const float *inv_level_sigma2, int n_levels,
                         float th, int chi2_gate, int32_t *best_idx /* [K*n] */, uint8_t *projected /* [K*n] or NULL */);

/* ------------------------------------------------------------------------- */
/* LoopClosing::ComputeSim3's two searches on the resident map points         */
/* ------------------------------------------------------------------------- */
/* One LEG of ORBmatcher::SearchBySim3 (src/ORBmatcher.cc:1251-1477): one direction of one candidate, the source key frame's
 * map points projected into the target key frame.  Rw / tw = the SOURCE key frame's GetRotation (row-major) / GetTranslation;
 * sR / t = source camera to target camera, i.e. sR21, t21 for the leg KF1 -> KF2 and sR12, t12 for KF2 -> KF1 (:1268-1270);
 * the rest is what the leg reads of the TARGET: fx fy cx cy, mnMinX .. mnMaxY, mfLogScaleFactor, mnScaleLevels.  The CALLER
 * composes the 12 floats of sR / t per direction: s12*R12, (1.0/s12)*R12.t() and -sR21*t12 go through OpenCV's scaled-matrix
 * and product routines, whose rounding depends on the OpenCV version and build, and have no place in a kernel. */
typedef struct orbfe_sim3_leg {
  float Rw[9], tw[3];
  float sR[9], t[3];
  float fx, fy, cx, cy;
  float min_x, max_x, min_y, max_y;
  float log_scale_factor;
  int32_t n_levels;
} orbfe_sim3_leg;

/* The prologue of SearchBySim3 (:1298-1340, :1379-1420) for n_legs (<= 128) legs in ONE kernel launch.  Leg l owns entries
 * [offsets[l], offsets[l+1]) of the concatenated slot[] / skip[] -- the source key frame's GetMapPointMatches() in slot space,
 * as orbfe_obsgraph_get_keyframe_points returns it: slot -1 = no map point; skip = vbAlreadyMatched.  offsets[0] = 0; offsets
 * never descend; a leg may be empty.  Outputs hold offsets[n_legs] entries; any may be NULL; valid = the point passes every
 * test; where it is 0, u / v / dist / level are 0.  IEEE binary32 (binary64 where stated), no contraction, sums left to right,
 * in this order:
 *   reject slot -1; reject skip[i] (NULL = none); reject flags & ORBFE_MP_BAD;
 *   c1 = ((Rw00*X + Rw01*Y) + Rw02*Z) + tw0 (rows 1, 2 likewise); c2 = ((sR00*c1x + sR01*c1y) + sR02*c1z) + t0 (likewise);
 *   reject c2z < 0; invz = 1/c2z (the reference's 1.0/z in double, rounded to float, is the same float quotient:
 *   53 >= 2*24 + 2); x = c2x*invz; y = c2y*invz; u = fx*x + cx; v = fy*y + cy;
 *   KeyFrame::IsInImage (src/KeyFrame.cc:653-656): keep only u >= min_x && u < max_x && v >= min_y && v < max_y -- the upper
 *   bounds are strict, and a NaN coordinate (c2 == 0) is rejected;
 *   dist = (float)sqrt(sum (double)c2_i^2) -- the norm of the camera-frame vector, NOT of P - Ow;
 *   reject dist < 0.8f*min || dist > 1.2f*max; there is no viewing-angle test;
 *   level = clamp(ceil(log((double)(max/dist)) / (double)log_scale_factor), 0, n_levels-1) with the target's values.
 * Only offsets, the slot list, the mask and the legs go up.  A slot below -1 or at or past the capacity, n_legs outside
 * 0 .. 128, offsets that do not start at 0 or descend, a leg whose n_levels is not 1 .. 64 and NULL offsets / slot / legs return
 * ORBFE_ERR_INVALID before anything is enqueued; n_legs == 0 or no point at all is ORBFE_OK with nothing touched. */
int orbfe_project_sim3(orbfe_mappoints *mp, int n_legs, const int32_t *offsets /* [n_legs + 1] */, const int32_t *slot,
                       const uint8_t *skip, const orbfe_sim3_leg *legs /* [n_legs] */, uint8_t *valid, float *u, float *v,
                       int32_t *level, float *dist);

/* SearchBySim3(pKF1, pKF2_k, vpMatches12_k, s12_k, R12_k, t12_k, th) for K (<= 64) candidates of ONE key frame KF1 as ONE call:
 * both directions of all K candidates are 2K legs of one orbfe_project_sim3 launch, which writes the query windows (centre
 * (u, v), radius th * scale_factors[level] of the leg's target, octaves [level-1, level]) where the window search reads them
 * and gathers KF1's descriptors once for all K; the 2K best-keypoint searches (bound TH_HIGH) follow in one launch; the
 * agreement check of :1461-1474 runs on the host over the one download.
 *   slot1[N1] = KF1's GetMapPointMatches() in slot space (-1 = none), N1 = KF1->n; candidate k owns [offsets2[k], offsets2[k+1])
 *   of slot2[], N2_k = KF2[k]->n entries; legs12[k] is the leg KF1 -> KF2_k (sR21, t21, KF2_k's intrinsics), legs21[k] the leg
 *   KF2_k -> KF1.  scale_factors1 / scale_factors2 are KF1's / the candidates' mvScaleFactors, n_levels entries each.
 *   matched12_in[k*N1 + i1] = the slot of vpMatches12_k[i1] at entry or -1 (NULL = none): vbAlreadyMatched1.
 *   vbAlreadyMatched2 is the union of already2 (by the position in slot2[], NULL = none) and -- when g and kf2_slot are given --
 *   GetIndexInKeyFrame from the observation rows on the device (:1288-1290): for every matched slot, the live entry whose
 *   kf == kf2_slot[k] marks its idx if idx < N2_k; a matched slot at or past g's point_capacity has no row.
 *   match12[k*N1 + i1] = i2 for mutually consistent pairs, else -1; n_found[k] = the return value.  What the caller does with
 *   a pair (vpMatches12[i1] = vpMapPoints2[i2]) stays with the caller.
 * With K = 1 the result equals orbfe_search_by_sim3 fed with orbfe_project_sim3's outputs and the table's descriptors, bit for
 * bit.  Beyond orbfe_project_sim3's checks: K outside 0 .. 64, N2_k != KF2[k]->n, a matched slot below -1 or at or past the
 * capacity, a kf2_slot outside the graph, a leg's n_levels above n_levels, bad views, NULL required arrays and handles on
 * different devices return ORBFE_ERR_INVALID before anything is enqueued; K == 0 is ORBFE_OK.  Takes g's serialisation, then
 * mp's. */
int orbfe_search_by_sim3_mappoints_multi(orbfe_mappoints *mp, orbfe_obsgraph *g /* or NULL */, const orbfe_frame_view *KF1,
                                         const int32_t *slot1 /* [N1] */, int n_candidates,
                                         const orbfe_frame_view *const *KF2 /* [K] */, const int32_t *offsets2 /* [K + 1] */,
                                         const int32_t *slot2, const orbfe_sim3_leg *legs12 /* [K] */,
                                         const orbfe_sim3_leg *legs21 /* [K] */, const int32_t *matched12_in /* [K*N1] or NULL */,
                                         const int32_t *kf2_slot /* [K], with g */, const uint8_t *already2 /* or NULL */,
                                         const float *scale_factors1, const float *scale_factors2, int n_levels, float th,
                                         int32_t *match12 /* [K*N1] */, int32_t *n_found /* [K] */);

/* ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) (src/ORBmatcher.cc:335-451, LoopClosing::ComputeSim3 over
 * mvpLoopMapPoints) as ONE call.  Its prologue (:366-405) is the Sim3 Fuse prologue term by term, so orbfe_project_fuse's
 * kernel runs it at K = 1 without a graph (pose = the caller's decomposition of Scw, as for orbfe_fuse_mappoints), writes the
 * windows and gathers the descriptors; the window search and the claim loop of :418-446 (TH_LOW) run behind it on the same
 * stream.  slot[] = vpPoints in slot space (no -1: the reference dereferences every entry); skip[i] = spAlreadyFound.count(pMP)
 * (NULL = none); matched[idx] = vpMatched[idx] != NULL at entry (NULL = none).  match[idx] = the POSITION IN slot[] of the point
 * newly given to keypoint idx of KF, or -1; *n_matches = the return value; projected[i] (optional) = the point passed the
 * prologue.  Equal to orbfe_search_by_projection_sim3 fed with orbfe_project_fuse's outputs and the table's descriptors, bit
 * for bit.  Argument errors as for orbfe_fuse_mappoints; n == 0 is ORBFE_OK with match cleared. */
int orbfe_search_by_projection_sim3_mappoints(orbfe_mappoints *mp, int n, const int32_t *slot, const uint8_t *skip,
                                              const orbfe_camera_pose *pose, const orbfe_frame_view *KF,
                                              const float *scale_factors, int n_levels, const uint8_t *matched, float th,
                                              int32_t *match, int32_t *n_matches, uint8_t *projected /* [n] or NULL */);

/* ---- Loop correction: the head of LoopClosing::CorrectLoop (src/LoopClosing.cc:514-604) and the map update at the tail
 * of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:787-852).  Sim3 records are the project's
 * qx qy qz qw tx ty tz s, binary64.  Poses are row-major 4 x 4 floats.
 *
 * The float cv::Mat products are restated as cv::gemm evaluates CV_32F operands (modules/core/src/matmul.cpp:
 * GEMMSingleMul<float, double>, the accumulator is double), `R * P + t` folded by cv::MatExpr into one gemm with
 * beta = 1 (modules/core/src/matop.cpp: MatOp_GEMM::add):
 *   D_ij = (float)( (double)A_i0 B_0j + (double)A_i1 B_1j + ... [+ (double)C_ij] ), added left to right.
 * A product of two binary32 values is exact in binary64, so contraction cannot change a bit.  SetPose, UpdateConnections,
 * Replace / AddObservation of :609-625, LoopConnections, the mutexes and the threads stay with the caller. ---- */

/* CorrectedSim3, NonCorrectedSim3 (:519-551) and the corrected poses (:590-596) of the K key frames of
 * mvpCurrentConnectedKFs.  Tiw[k] = GetPose(), Twc_cur = mpCurrentKF->GetPoseInverse(), cur = its index in the list, Scw =
 * mg2oScw.  Tic = Tiw * Twc as above; g2o::Sim3(R, t, 1) is Eigen's Quaterniond(Matrix3d); g2oSic * mg2oScw is g2o's
 * product (sim3.h:266-272, no normalisation); Tiw_corrected = [R | t * (1 / s)] as floats.  corrected[cur] is Scw bit for
 * bit; noncorrected[., 7] is exactly 1.  A non-finite input, a scale <= 0 and cur outside [0, K) return ORBFE_ERR_INVALID
 * with nothing written.  Host code: needs no device. */
int orbfe_correct_loop_sim3s(int K, const float *Tiw /* [K*16] */, const float *Twc_cur /* [16] */, int cur, const double *Scw /* [8] */,
                             double *corrected /* [K*8] */, double *noncorrected /* [K*8] */, float *Tiw_corrected /* [K*16] */);
/* The point loop of :558-587 on arrays: key frame k lists point[offsets[k] .. offsets[k+1]) (-1 = NULL); skip[p] =
 * isBad() || mnCorrectedByKF == current (NULL = none).  corrected_ref[p] = the lowest k whose list names p (-1: untouched,
 * xw copied through); xw_out[p] = corrected[k]^-1 .map( noncorrected[k] .map(xw[p]) ), the arithmetic of
 * orbfe_essential_graph_correct_points: binary64, stored as float.  Deviation: the reference walks std::map<KeyFrame*, ..>
 * in pointer order; here the order is the caller's list (ascending mnId is recommended).  Host code: needs no device. */
int orbfe_correct_loop_points(int K, const double *corrected, const double *noncorrected, const int32_t *offsets /* [K+1] */,
                              const int32_t *point, int n_points, const float *xw, const uint8_t *skip /* or NULL */, float *xw_out,
                              int32_t *corrected_ref);
/* The same loop, with MapPoint::UpdateNormalAndDepth (:586), on the resident state: g with key-frame rows enabled holds
 * mvpMapPoints, the observation rows, the bad flags, the reference key frames and Ow; mp holds position, normal and range.
 * kf_slot[K]: the key frames in visiting order.  Deviation: the reference visits std::map<KeyFrame*, ..> in pointer order,
 * which differs from run to run; the call takes any order, ascending mnId is recommended (the row-order deviation of
 * orbfe_obsgraph is the same kind).  skip_slot[n_skip]: the points with mnCorrectedByKF == current.
 *   Claim.  Key frames in list order, a row's entries in idx order; an entry is passed over when it is -1, when the point is
 *   bad or was never set, or when the point is in the skip list.  A point belongs to the lowest position
 *   k * kf_row_width + idx that names it -- an integer minimum, never arrival order.  A kf slot named twice contributes
 *   nothing the second time (and its first Ow_corrected is the one kept).
 *   Correct.  The claimed point's position in mp is rewritten in place, bit-equal to orbfe_correct_loop_points.
 *   Normal and depth.  orbfe_obsgraph_update_normal_depth's restatement at the new position, with one rule added: an
 *   observing key frame whose place in the list is BELOW the claimant's uses Ow_corrected[place] (the reference has called
 *   SetPose on it by then, :600); every other observer -- the claimant itself, later places, key frames outside the list --
 *   uses the centre the graph holds.  The same rule picks the reference key frame's centre for the distance.  valid = 0 as
 *   for orbfe_obsgraph_update_normal_depth: the position is still corrected, normal and range keep what they hold.
 * slot_out[]: the claimed slots in claim order; ref_out[]: the claimant's place in the list (mnCorrectedReference; the
 * ref_vertex of orbfe_essential_graph_correct_mappoints); valid_out[] (may be NULL); *count.  A count above `capacity`
 * returns ORBFE_ERR_CAPACITY with *count set and both tables untouched.  On success the K key frames' Ow in g, host mirror
 * and device, are Ow_corrected (the caller's GetCameraCenter() after SetPose(Tiw_corrected)): no set_keyframes is needed.
 * ORBFE_ERR_INVALID before anything is enqueued: a kf slot out of range or never set, rows not enabled, K * kf_row_width
 * >= 2^31, a non-finite record or centre, a scale <= 0, a skip slot out of range, handles on different devices or g with
 * more point slots than mp, and a reference entry of a point the rows name whose octave is not below n_levels.  Takes g's
 * serialisation, then mp's; complete on return. */
int orbfe_correct_loop_mappoints(orbfe_obsgraph *g, orbfe_mappoints *mp, int K, const int32_t *kf_slot, const double *corrected,
                                 const double *noncorrected, const float *Ow_corrected /* [K*3] */, int n_skip,
                                 const int32_t *skip_slot, const float *scale_factors, int n_levels, int capacity, int32_t *slot_out,
                                 int32_t *ref_out, uint8_t *valid_out /* or NULL */, int32_t *count);

/* The spanning-tree walk of :788-815 on indices: origin[] = mvpKeyFrameOrigins, the children of key frame k =
 * child[child_offsets[k] .. child_offsets[k+1]) (their order is immaterial: a child's result depends on its parent alone),
 * Tcw / Twc = GetPose() / GetPoseInverse() at entry, in_gba[k] = (mnBAGlobalForKF == nLoopKF) at entry, Tcw_gba[k] = mTcwGBA,
 * read where in_gba is set.  A child that was not in the GBA gets (:803-805) Tchildc = Tcw[child] * Twc[parent] and
 * mTcwGBA = Tchildc * mTcwGBA[parent], two float products as above.  Tcw_new[k] = mTcwGBA after the walk (Tcw[k] for a key
 * frame that was neither reached nor visited), reached[k] = the flag after the walk, visited[k] = the key frame was in the
 * walk and receives SetPose(Tcw_new[k]) with mTcwBefGBA = Tcw[k].  An origin that was not in the GBA keeps its flag and, as in
 * the reference (:813), receives whatever Tcw_gba holds for it: Tcw_gba is read for every origin as well.  ORBFE_ERR_INVALID
 * with nothing written: an index out of range, a non-finite pose that would be read, a key frame visited twice (a cycle, or
 * two parents).  Host code: needs no device. */
int orbfe_gba_propagate_keyframes(int n, int n_origins, const int32_t *origin, const int32_t *child_offsets /* [n+1] */,
                                  const int32_t *child, const float *Tcw, const float *Twc, const uint8_t *in_gba, const float *Tcw_gba,
                                  float *Tcw_new, uint8_t *reached, uint8_t *visited);
/* The point loop of :818-852 on arrays.  moved[p] = 0: skipped (the point is bad, its reference key frame was not reached,
 * or -- deviation -- ref_kf[p] = -1, where the reference would dereference NULL) and xw is copied through; 1: the point
 * took pos_gba (in_gba[p] = mnBAGlobalForKF == nLoopKF); 2: it was moved through its reference key frame,
 *   Xc = Rcw_bef * P + tcw_bef;  P' = Rwc_new * Xc + twc_new,  each ONE gemm with beta = 1 as above:
 *   Xc_i = (float)( (double)R_i0 P_0 + (double)R_i1 P_1 + (double)R_i2 P_2 + (double)t_i ), added left to right.
 * Tcw_bef[k] = mTcwBefGBA, Twc_new[k] = GetPoseInverse() after SetPose, read where reached[k].  Host code. */
int orbfe_gba_update_points(int n_points, const float *xw, const uint8_t *bad, const uint8_t *in_gba, const float *pos_gba,
                            const int32_t *ref_kf, int n_kf, const uint8_t *reached, const float *Tcw_bef, const float *Twc_new,
                            float *xw_out, uint8_t *moved);
/* The same on the resident state: slot[n] = the caller's GetAllMapPoints (distinct slots), in_gba / pos_gba aligned with it;
 * kf_slot[m] a compact list of distinct kf slots with reached / Tcw_bef / Twc_new aligned.  The bad flag and the reference
 * kf slot come from g's point record (a slot never set counts as bad); a reference key frame that is not in the compact
 * list counts as not reached.  Positions in mp are rewritten in place, bit-equal to orbfe_gba_update_points; moved[n] as
 * there.  Normal and range are the caller's next orbfe_obsgraph_update_normal_depth_mappoints (the reference does not
 * update them here either).  A slot or kf slot out of range or named twice, a non-finite pose or position that would be
 * read, handles on different devices return ORBFE_ERR_INVALID before anything is enqueued.  Takes g's serialisation, then
 * mp's; complete on return. */
int orbfe_gba_update_mappoints(orbfe_obsgraph *g, orbfe_mappoints *mp, int n, const int32_t *slot, const uint8_t *in_gba,
                               const float *pos_gba, int m, const int32_t *kf_slot, const uint8_t *reached, const float *Tcw_bef,
                               const float *Twc_new, uint8_t *moved);

/* ---- Where stereo and RGB-D map points are born: Tracking::StereoInitialization (src/Tracking.cc:563-578, mode ALL),
 * the depth-sorted loop of Tracking::CreateNewKeyFrame (:1182-1234, mode KEYFRAME) and the same loop of
 * Tracking::UpdateLastFrame (:899-949, mode TEMPORAL: the visual-odometry points of localisation mode, made by the Frame
 * constructor of MapPoint, src/MapPoint.cc:46-71).  IEEE binary32 with no contraction, binary64 where stated.
 *   Selection.  Candidates are the keypoints with depth > 0: NaN, zero and negative depths are none, +inf is one.  ALL: the
 *   candidates in ascending index, each created, the occupied mask not read.  KEYFRAME / TEMPORAL: the candidates ordered as
 *   std::sort orders pair<float, int> (ascending z, ties by ascending index); candidate j = 0, 1, .. is created unless
 *   occupied[i] (mvpMapPoints[i] && Observations() >= 1); after handling candidate j the walk stops when z_j > th_depth &&
 *   j + 1 > 100 (nPoints grows in both branches of :1213-1229), so z == th_depth goes on and 100 or fewer candidates are
 *   all handled.  KEYFRAME also returns cleared[i] = 1 for a created keypoint with stale[i] set (a point with
 *   Observations() < 1, :1207-1211: the caller's mvpMapPoints[i] is dropped); occupied and stale on one keypoint is an error.
 *   Either mask may be NULL (none set).
 *   Frame::UnprojectStereo (src/Frame.cc:713-727).  x = ((u - cx) * z) * invfx, y likewise, u / v = mvKeysUn[i].pt, invfx =
 *   1.0f / fx; P_r = (float)((double)Rwc_r0 x + (double)Rwc_r1 y + (double)Rwc_r2 z + (double)Ow_r), added left to right, Rwc the
 *   exact transpose of pose.Rcw: the CV_32F gemm-with-beta restatement of the loop correction above (and, as there, not
 *   checked against OpenCV's small-matrix path, whose source was not at hand).  A NaN that an infinite depth produces has
 *   no defined sign or payload.
 *   Normal and range.  orbfe_obsgraph_update_normal_depth for a row of one entry: d = P - C; nrm = sqrt(sum (double)d_i^2);
 *   normal_i = (0.0f + d_i * (float)(1.0 / nrm)) * (float)(1.0 / 1); dist = (float)nrm; max_dist = dist *
 *   scale_factors[octave_i]; min_dist = max_dist / scale_factors[n_levels - 1].  ALL / KEYFRAME: C is the key frame's centre;
 *   TEMPORAL: C = pose.Ow (mNormalVector / cv::norm(mNormalVector) of the Frame constructor is the same expression).
 *   The descriptor is the frame's row i.  Flags: not bad; ORBFE_MP_OBSERVED in ALL / KEYFRAME, clear in TEMPORAL (nObs == 0). */
#define ORBFE_STEREO_ALL 0
#define ORBFE_STEREO_KEYFRAME 1
#define ORBFE_STEREO_TEMPORAL 2
/* The definition, on arrays: x / y / octave / depth [n], occupied / stale [n] or NULL, centre [3] = C.  created_idx: the
 * keypoint indices in creation order, *n_created of them, with pos / normal [.,3] and min_dist / max_dist aligned; cleared
 * [n] (may be NULL); *n_walked: the candidates handled before the stop.  More created points than `capacity` returns
 * ORBFE_ERR_CAPACITY with both counts set and no array written.  ORBFE_ERR_INVALID with nothing written: n < 0 or
 * n > 16384, an unknown mode, n_levels outside 1 .. 256, an octave outside [0, n_levels), a non-finite pose or centre,
 * fx == 0 or fy == 0, a keypoint both occupied and stale, NULL arrays.  Host code: needs no device. */
int orbfe_stereo_points_select(int n, const float *x, const float *y, const int32_t *octave, const float *depth,
                               const uint8_t *occupied, const uint8_t *stale, const orbfe_camera_pose *pose, float th_depth, int mode,
                               const float *scale_factors, int n_levels, const float *centre, int capacity, int32_t *created_idx,
                               float *pos, float *normal, float *min_dist, float *max_dist, uint8_t *cleared, int32_t *n_created,
                               int32_t *n_walked);
/* nTrackedClose / nNonTrackedClose of Tracking::NeedNewKeyFrame (:1100-1114): over the keypoints with 0 < depth < th_depth,
 * strict on both sides, has_point[i] && !outlier[i] counts as tracked, every other one as not tracked.  Host code. */
int orbfe_count_close_points(int n, const float *depth, const uint8_t *has_point, const uint8_t *outlier, float th_depth,
                             int32_t *n_tracked_close, int32_t *n_non_tracked_close);
/* The same selection and arithmetic on the resident state, in one call: keypoints, octaves, descriptors and the stereo bit
 * are read from the resident frame F (n must be its keypoint count); the depth array, the two masks, the slot list, the pose
 * and the level table go up; created point number j takes new_slot[j] (capacity entries) and its position, normal, range,
 * descriptor and flags are written straight into mp's rows, bit-equal to orbfe_stereo_points_select with C = the centre g
 * holds for kf_slot (TEMPORAL: pose.Ow) -- and so to a later orbfe_obsgraph_update_normal_depth_mappoints on the new slots.
 * One kernel (the keys bits(z) << 32 | i sorted in one workgroup's LDS), one copy back: created_idx / created_slot
 * [*n_created], cleared [n], *n_walked.  More created points than `capacity` returns ORBFE_ERR_CAPACITY with *n_created the
 * needed count and neither table touched.  In modes ALL and KEYFRAME the map bookkeeping of :1216-1221 is then applied to
 * g's mirror in creation order: set_points(bad = 0, ref = kf_slot), add_observations(slot, kf_slot, idx, octave, the frame's
 * own mvuRight >= 0 bit) and, when key-frame rows are enabled, assign_keyframe_points.  TEMPORAL reads no graph (g may be
 * NULL).  ORBFE_ERR_INVALID before anything is enqueued: what orbfe_stereo_points_select rejects; n != F's count; g NULL
 * outside TEMPORAL; kf_slot out of range or never set; a new slot out of range, named twice, at or past g's point capacity,
 * or whose graph row is live (only a slot never set, or bad with an empty row, is free); key-frame rows enabled and
 * kf_slot's row shorter than n; handles on different devices.  n == 0 or no candidate is ORBFE_OK with zero counts and no
 * launch.  Takes g's serialisation, then mp's; complete on return. */
int orbfe_create_stereo_points(orbfe_mappoints *mp, orbfe_obsgraph *g /* NULL only in TEMPORAL */, const orbfe_frame *F, int kf_slot,
                               const orbfe_camera_pose *pose, int n, const float *depth, const uint8_t *occupied,
                               const uint8_t *stale, float th_depth, int mode, const float *scale_factors, int n_levels,
                               const int32_t *new_slot, int capacity, int32_t *created_idx, int32_t *created_slot, uint8_t *cleared,
                               int32_t *n_created, int32_t *n_walked);

/* ---- Where triangulated map points are born: the birth at the tail of LocalMapping::CreateNewMapPoints' pair loop
 * (src/LocalMapping.cc:283-501; the neighbour loop :283, the pair loop :333, the birth :484-500), the only birth a monocular
 * map has after initialisation.  IEEE binary32 with no contraction, binary64 where stated.
 *   Per pair.  Status and position are orbfe_triangulate_matches_multi's, by the same code: the position is its x3d, bit
 *   for bit.  cam.Ow is read where that call reads it (UnprojectStereo and the scale-consistency test, :465-481) and nowhere
 *   else.
 *   Who and in what order.  Pair (k, i1) makes a point when its status is ORBFE_TRI_CREATED and k is the smallest neighbour
 *   index with a CREATED pair for i1 -- the `winner` rule above (AddMapPoint at :489 takes i1 out of every later
 *   neighbour's search, src/ORBmatcher.cc:800-803).  Creation order is ascending (k, i1): the reference's two loops, with
 *   vMatchedIndices ascending in idx1.  Created point number w takes new_slot[w].
 *   Descriptor.  MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:269-333) at N = 2: both medians are the
 *   self-distance 0 and `<` is strict, so the first entry of the row wins -- the key frame with the smaller mnId in the
 *   ascending-mnId row order of orbfe_obsgraph.  The descriptor is that key frame's row (i1 of key frame 1, or i2 of the
 *   neighbour): orbfe_obsgraph_distinctive_descriptors for a row of two entries.
 *   Normal and range.  orbfe_obsgraph_update_normal_depth for the row of two entries A, B in ascending mnId, operation by
 *   operation: d = P - C; a = (float)(1.0 / sqrt(sum (double)d_i^2)); normal_i = ((0.0f + dA_i * aA) + dB_i * aB) *
 *   (float)(1.0 / 2).  The reference key frame is key frame 1 (mpRefKF = mpCurrentKeyFrame, :484): dist = (float)|P - C1|,
 *   max_dist = dist * scale_factors[octave of keypoint i1], min_dist = max_dist / scale_factors[n_levels - 1].  In the
 *   resident call C1 / C2 are the centres the graph holds for the kf slots -- the graph is the truth, as for
 *   orbfe_create_stereo_points -- whatever cam.Ow says.
 *   Flags: not bad, ORBFE_MP_OBSERVED. */
/* The definition, on arrays: match12 / status / x3d as orbfe_triangulate_matches_multi takes and returns them ([k*n1 + i1]);
 * kf1_id / kf2_id [K] the key frames' mnIds, centre1 [3] / centre2 [K*3] their centres, octave1 [n1] key frame 1's octaves.
 * created_k / created_i1 / created_i2 [*n_created] in creation order with pos / normal [.,3], min_dist / max_dist and
 * desc_from (0: key frame 1's descriptor row i1, 1: the neighbour's row i2) aligned.  More created points than `capacity`
 * returns ORBFE_ERR_CAPACITY with *n_created set and no array written.  ORBFE_ERR_INVALID with nothing written: n1 outside
 * [0, 16384], n_neighbours outside [0, 64], n_levels outside (0, ORBFE_MAX_LEVELS], a negative capacity or id, two equal ids,
 * a non-finite centre, a match outside [-1, 16384), a status above ORBFE_TRI_SCALE or one that disagrees with match12 about
 * which pairs exist, a keypoint i2 named twice within one neighbour, a created keypoint's octave outside [0, n_levels), NULL
 * arrays.  Host code: needs no device. */
int orbfe_triangulated_points_select(int n1, int n_neighbours, const int32_t *match12, const uint8_t *status, const float *x3d,
                                     int64_t kf1_id, const int64_t *kf2_id, const float *centre1, const float *centre2,
                                     const int32_t *octave1, const float *scale_factors, int n_levels, int capacity,
                                     int32_t *created_k, int32_t *created_i1, int32_t *created_i2, float *pos, float *normal,
                                     float *min_dist, float *max_dist, uint8_t *desc_from, int32_t *n_created);
/* The triangulation and the birth on the resident state, in one call.  Keypoints, octaves, u_right and descriptors are read
 * from the resident frames; the pair records (compacted from match12 in (k, i1) order), the K + 1 cameras, the K + 1 centres
 * and mnIds g holds for kf1_slot / kf2_slot[k], the slot list and the level tables go up; one copy brings back the lists,
 * the counts and the statuses.  Two launches on g's stream: one lane per pair solves it (as orbfe_triangulate_matches_multi)
 * and names the winner by an integer minimum; one workgroup then places the kept pairs by prefix sums over the list and
 * writes position, normal, range, descriptor and flags straight into mp's rows -- bit-equal to
 * orbfe_triangulated_points_select on orbfe_triangulate_matches_multi's outputs, and so to orbfe_mappoints_update with
 * those values followed by orbfe_obsgraph_distinctive_descriptors_mappoints and
 * orbfe_obsgraph_update_normal_depth_mappoints on the new slots.  The map bookkeeping of :484-492 is then applied to g's
 * mirror in creation order: set_points(bad = 0, ref = kf1_slot), add_observations(slot, kf1_slot, i1, octave1, stereo1) and
 * (slot, kf2_slot[k], i2, octave2, stereo2) with the frames' own u_right >= 0 bit, and, when key-frame rows are enabled,
 * assign_keyframe_points for both key frames (it overwrites, as AddMapPoint does).
 * Outputs: created_k / created_i1 / created_i2 / created_slot [*n_created]; status [K*n1] as orbfe_triangulate_matches_multi
 * (may be NULL); n_created_per_neighbour [K] = the points made with neighbour k (their sum is *n_created).  More created
 * points than `capacity` returns ORBFE_ERR_CAPACITY with *n_created the needed count, the other counts and status set and
 * neither table touched.  n_neighbours == 0 or no pair is ORBFE_OK with zero counts and no launch.
 * ORBFE_ERR_INVALID before anything is enqueued: what orbfe_triangulate_matches_multi rejects of its inputs; a keypoint i2
 * named twice within one neighbour; kf1_slot or a kf2_slot out of range, never set, bad, or named twice (kf1_slot among
 * them); two key frames with the same mnId; a new slot out of range, named twice, at or past g's point capacity, or whose
 * graph row is live; key-frame rows enabled and a row shorter than its frame's keypoint count; handles or frames on different devices; NULL arrays.  Takes g's serialisation, then mp's; complete on
 * return. */
int orbfe_create_triangulated_points(orbfe_mappoints *mp, orbfe_obsgraph *g, const orbfe_frame *kf1, int kf1_slot,
                                     const orbfe_keyframe_camera *cam1, int n_neighbours, const orbfe_frame *const *kf2,
                                     const int32_t *kf2_slot, const orbfe_keyframe_camera *cam2 /*[K]*/,
                                     const int32_t *match12 /*[K*n1]*/, const float *scale_factors, const float *level_sigma2,
                                     int n_levels, float ratio_factor, const int32_t *new_slot, int capacity,
                                     int32_t *created_k, int32_t *created_i1, int32_t *created_i2, int32_t *created_slot,
                                     uint8_t *status /*[K*n1], may be NULL*/, int32_t *n_created_per_neighbour /*[K]*/,
                                     int32_t *n_created);

#ifdef __cplusplus
}
#endif
#endif /* ORBFE_H */
