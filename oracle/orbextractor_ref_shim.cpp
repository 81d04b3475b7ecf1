// orbextractor_ref_shim.cpp -- C entry points over the REFERENCE's own src/ORBextractor.cc, which oracle/Makefile
// (target `ref`) compiles where it lies, unmodified, against the OpenCV double in oracle/ref_cv/ and links with this
// file and orb_oracle.c into oracle/_ref/liborbextractor_ref.so.  Test infrastructure only.
//
// What then RUNS FROM THE REFERENCE'S TEXT: the constructor tables (scale tables, quotas, umax), ComputePyramid (ROI
// and border structure, level sizes), ComputeKeyPointsOctTree (cell geometry, the second FAST call), DistributeOctTree,
// ExtractorNode::DivideNode, IC_Angle, computeOrbDescriptor (pattern rotation, cvRound of the rotated pattern, libm's
// cosf / sinf) and the level order and rescale of operator().
//
// What does NOT: the nine symbols that file leaves undefined are OpenCV's, and OpenCV is absent.  They are defined
// here by calling the oracle's primitives (orc_cvround, orc_fast_atan2, orc_fast_nms, orc_gaussian_blur7_spec,
// orc_resize_linear), so the ARITHMETIC of cvRound / cvFloor / cvCeil, fastAtan2, FAST, GaussianBlur and resize stays the
// oracle's restatement; copyMakeBorder is written here (reflect-101 of the ROI).  None of the reference's bodies is
// repeated in this file.
//
// ONE MORE THING IS PINNED HERE, and it is a finding about the reference: DistributeOctTree sorts
// pair<int, ExtractorNode*> to split the fullest nodes first, so among nodes that hold EQUALLY MANY keypoints the
// order is that of the list nodes' ADDRESSES, and when N is reached in the middle of that pass (the early `break`)
// the result depends on it.  Under the C library's allocator the same call returns different keypoints depending on
// what the heap did before.  This library therefore replaces operator new / delete for itself (-Bsymbolic, nothing
// crosses its boundary) with a bump arena during its calls: addresses grow in allocation order and are never reused,
// which makes "higher address" mean "created later" -- the order the oracle and the product use, (count, creation
// order) -- and the reference's result a function of its arguments.
#include <sys/mman.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "ORBextractor.h"  // -I <reference>/include; pulls the double in through <opencv/cv.h>
#include "orb_oracle.h"

static int g_blur_spec = 0;    // which GaussianBlur arithmetic cv::GaussianBlur runs (orc_gaussian_blur7_spec)
static int g_fast_stats[4];    // cv::FAST [calls, non-empty results] at iniThFAST, then at any other threshold
static int g_ini_thr = -1;

static void die(const char* what) {
  std::fprintf(stderr, "orbextractor_ref_shim: %s\n", what);
  std::abort();
}

// ---- the bump arena behind this library's operator new (see the header) ----
static const size_t kArenaBytes = (size_t)4 << 30;  // address space only: pages are committed when touched
static char* g_arena = 0;
static size_t g_arena_used = 0;
static bool g_arena_on = false;

static void arena_release_to(size_t mark) {  // everything allocated above `mark` must be dead
  if (g_arena && g_arena_used > mark) {
    const size_t from = (mark + 4095) & ~(size_t)4095;
    if (g_arena_used > from) madvise(g_arena + from, g_arena_used - from, MADV_DONTNEED);
  }
  g_arena_used = mark;
}
struct ArenaScope {  // allocations of this scope come from the arena; `release` gives them back at its end
  size_t mark;
  bool release;
  explicit ArenaScope(bool rel) : mark(g_arena_used), release(rel) {
    if (!g_arena) {
      void* p = mmap(0, kArenaBytes, PROT_READ | PROT_WRITE, MAP_PRIVATE | MAP_ANONYMOUS | MAP_NORESERVE, -1, 0);
      if (p == MAP_FAILED) die("cannot reserve the allocation arena");
      g_arena = (char*)p;
    }
    g_arena_on = true;
  }
  ~ArenaScope() {
    g_arena_on = false;
    if (release) arena_release_to(mark);
  }
};

void* operator new(size_t n) {
  if (!g_arena_on) {
    void* p = std::malloc(n ? n : 1);
    if (!p) throw std::bad_alloc();
    return p;
  }
  n = (n + 15) & ~(size_t)15;
  if (g_arena_used + n > kArenaBytes) die("allocation arena exhausted");
  void* p = g_arena + g_arena_used;
  g_arena_used += n;
  return p;
}
void* operator new[](size_t n) { return operator new(n); }
void operator delete(void* p) noexcept {
  if (p && !(g_arena && (char*)p >= g_arena && (char*)p < g_arena + kArenaBytes)) std::free(p);
}
void operator delete[](void* p) noexcept { operator delete(p); }
void operator delete(void* p, size_t) noexcept { operator delete(p); }
void operator delete[](void* p, size_t) noexcept { operator delete(p); }

int cvRound(double v) { return orc_cvround(v); }
int cvFloor(double v) { int i = (int)v; return i - (i > v); }
int cvCeil(double v) { int i = (int)v; return i + (i < v); }

namespace cv {

float fastAtan2(float y, float x) { return orc_fast_atan2(y, x); }

// Keypoints of the sub-image in OpenCV's row-major order, pt relative to the sub-image, response = score,
// size 7, the rest KeyPoint's defaults; reads through the view's step.
void FAST(InputArray image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmax) {
  if (!nonmax) die("cv::FAST without non-maximum suppression is not provided");
  const Mat m = image.getMat();
  keypoints.clear();
  const int which = threshold == g_ini_thr ? 0 : 2;
  g_fast_stats[which]++;
  if (m.cols < 7 || m.rows < 7) return;
  const int cap = m.cols * m.rows;
  std::vector<int> xs(cap), ys(cap), sc(cap);
  const int n = orc_fast_nms(m.data, m.cols, m.rows, (int)m.step, threshold, &xs[0], &ys[0], &sc[0], cap);
  for (int i = 0; i < n; i++) keypoints.push_back(KeyPoint((float)xs[i], (float)ys[i], 7.f, -1, (float)sc[i]));
  if (n > 0) g_fast_stats[which + 1]++;
}

// Called in place on a clone; the oracle's blur finishes its horizontal pass before it writes dst.
void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY, int borderType) {
  Mat s = src.getMat();
  dst.create(s.rows, s.cols, CV_8UC1);
  Mat d = dst.getMat();
  if (ksize.width != 7 || ksize.height != 7 || sigmaX != 2 || sigmaY != 2 || borderType != BORDER_REFLECT_101)
    die("cv::GaussianBlur: only 7x7, sigma 2, BORDER_REFLECT_101 is provided");
  orc_gaussian_blur7_spec(s.data, s.cols, s.rows, (int)s.step, d.data, (int)d.step, g_blur_spec);
}

// dst.create() is a no-op when dst already has dsize: mvImagePyramid[level] is a view into `temp` and must stay one.
void resize(InputArray src, OutputArray dst, Size dsize, double fx, double fy, int interpolation) {
  if (fx != 0 || fy != 0 || interpolation != INTER_LINEAR) die("cv::resize: only dsize + INTER_LINEAR is provided");
  const Mat s = src.getMat();
  dst.create(dsize.height, dsize.width, CV_8UC1);
  Mat d = dst.getMat();
  orc_resize_linear(s.data, s.cols, s.rows, (int)s.step, d.data, d.cols, d.rows, (int)d.step);
}

static int reflect101(int i, int n) {
  if (n == 1) return 0;
  while (i < 0 || i >= n) i = i < 0 ? -i : 2 * (n - 1) - i;
  return i;
}

// dst keeps its buffer when it already has the bordered size; the interior is copied only when src is not already
// that interior (levels >= 1 pass the view of dst itself); the border is reflect-101 of the src view alone, which is
// what BORDER_ISOLATED asks for and what a src that is no view of a larger image gets anyway.
void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType,
                    const Scalar&) {
  if ((borderType & ~BORDER_ISOLATED) != BORDER_REFLECT_101) die("cv::copyMakeBorder: only BORDER_REFLECT_101 is provided");
  const Mat s = src.getMat();
  dst.create(s.rows + top + bottom, s.cols + left + right, CV_8UC1);
  Mat d = dst.getMat();
  uchar* inner = d.data + (size_t)top * d.step + left;
  if (inner != s.data)
    for (int y = 0; y < s.rows; y++) std::memmove(inner + (size_t)y * d.step, s.ptr(y), s.cols);
  for (int y = 0; y < d.rows; y++) {
    const uchar* from = inner + (size_t)reflect101(y - top, s.rows) * d.step;
    uchar* to = d.ptr(y);
    const bool border_row = y < top || y >= top + s.rows;
    for (int x = 0; x < d.cols; x++)
      if (border_row || x < left || x >= left + s.cols) to[x] = from[reflect101(x - left, s.cols)];
  }
}

void KeyPointsFilter::retainBest(std::vector<KeyPoint>&, int) {
  die("cv::KeyPointsFilter::retainBest: only the uncalled ComputeKeyPointsOld uses it");
}

}  // namespace cv

namespace {

struct RefExtractor : ORB_SLAM2::ORBextractor {  // reaches the protected members
  RefExtractor(int n, float s, int l, int i, int m) : ORB_SLAM2::ORBextractor(n, s, l, i, m) {}
  void tables(int32_t* quota, float* sf, float* isf, float* s2, float* is2, int32_t* um) const {
    for (int l = 0; l < nlevels; l++) {
      quota[l] = mnFeaturesPerLevel[l];
      sf[l] = mvScaleFactor[l]; isf[l] = mvInvScaleFactor[l];
      s2[l] = mvLevelSigma2[l]; is2[l] = mvInvLevelSigma2[l];
    }
    for (size_t v = 0; v < umax.size() && v < 16; v++) um[v] = umax[v];
  }
  std::vector<cv::KeyPoint> distribute(const std::vector<cv::KeyPoint>& k, int minX, int maxX, int minY, int maxY,
                                       int N, int level) {
    return DistributeOctTree(k, minX, maxX, minY, maxY, N, level);
  }
};

RefExtractor* g_last = 0;  // the extractor of the last ref_extract call: ref_pyramid_level reads its mvImagePyramid

}  // namespace

extern "C" {

void ref_set_blur_spec(int spec) { g_blur_spec = spec; }

// [calls, non-empty results] of cv::FAST at iniThFAST and at minThFAST during the last ref_extract
void ref_fast_stats(int32_t* out4) { for (int i = 0; i < 4; i++) out4[i] = g_fast_stats[i]; }

// ORBextractor(params)(image, Mat(), keypoints, descriptors): keypoints as the 28-byte records (cv::KeyPoint's layout),
// descriptors as rows of 32 bytes.  Returns 0, or -1 when more than `capacity` keypoints came out (*n_out holds them).
int ref_extract(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, const uint8_t* image, int w,
                int h, int stride, int blur_spec, orc_keypoint* kps, uint8_t* desc, int capacity, int* n_out) {
  static_assert(sizeof(cv::KeyPoint) == sizeof(orc_keypoint), "keypoint record layout");
  delete g_last;
  g_last = 0;
  arena_release_to(0);
  ArenaScope arena(false);  // kept until the next call: ref_pyramid_level reads g_last
  g_last = new RefExtractor(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
  g_blur_spec = blur_spec;
  std::memset(g_fast_stats, 0, sizeof g_fast_stats);
  g_ini_thr = iniThFAST;
  cv::Mat img(h, w, CV_8UC1), mask, descriptors;
  for (int y = 0; y < h; y++) std::memcpy(img.ptr(y), image + (size_t)y * stride, w);
  std::vector<cv::KeyPoint> keys;
  (*g_last)(img, mask, keys, descriptors);
  *n_out = (int)keys.size();
  if (keys.empty()) return descriptors.empty() ? 0 : -2;  // _descriptors.release()
  if ((int)keys.size() > capacity) return -1;
  if (descriptors.rows != (int)keys.size() || descriptors.cols != 32) return -2;
  std::memcpy(kps, &keys[0], keys.size() * sizeof(orc_keypoint));
  for (int i = 0; i < descriptors.rows; i++) std::memcpy(desc + (size_t)i * 32, descriptors.ptr(i), 32);
  return 0;
}

// mvImagePyramid[level] of the last ref_extract; border > 0 reads that many pixels of the surrounding `temp` as well
// (at most EDGE_THRESHOLD = 19; the view's data pointer sits inside that buffer).
int ref_pyramid_level(int level, int border, uint8_t* dst, int dst_stride, int* w, int* h) {
  if (!g_last || level < 0 || level >= (int)g_last->mvImagePyramid.size() || border < 0 || border > 19) return -1;
  const cv::Mat& m = g_last->mvImagePyramid[level];
  *w = m.cols; *h = m.rows;
  if (dst)
    for (int y = -border; y < m.rows + border; y++)
      std::memcpy(dst + (size_t)(y + border) * dst_stride, m.data + (ptrdiff_t)y * (ptrdiff_t)m.step - border,
                  m.cols + 2 * border);
  return 0;
}

// constructor tables: quota / the four scale tables hold nlevels entries, umax 16
int ref_tables(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int32_t* quota, float* sf,
               float* isf, float* s2, float* is2, int32_t* umax16) {
  ArenaScope arena(true);
  RefExtractor e(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST);
  e.tables(quota, sf, isf, s2, is2, umax16);
  return e.GetLevels();
}

// DistributeOctTree on n candidates (coordinates relative to (minX, minY)); out_idx receives the indices of the
// returned keypoints into the input, in the order of the returned vector.  Returns their number.
int ref_distribute_octtree(const float* xs, const float* ys, const float* resp, int n, int minX, int maxX, int minY,
                           int maxY, int N, int level, int32_t* out_idx, int cap) {
  ArenaScope arena(true);
  RefExtractor e(N > 0 ? N : 1, 1.2f, 1, 20, 7);
  std::vector<cv::KeyPoint> in(n);
  for (int i = 0; i < n; i++) in[i] = cv::KeyPoint(xs[i], ys[i], 7.f, -1, resp[i], 0, i);
  const std::vector<cv::KeyPoint> out = e.distribute(in, minX, maxX, minY, maxY, N, level);
  for (size_t i = 0; i < out.size() && (int)i < cap; i++) out_idx[i] = out[i].class_id;
  return (int)out.size();
}

}  // extern "C"
