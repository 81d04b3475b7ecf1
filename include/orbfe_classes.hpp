// orbfe_classes.hpp -- header-only C++ host layer over the C-ABI (orbfe.h), OpenCV-free.
//
// Mirrors the reference's operator/plugin interface for the hot path with the same names,
// argument meaning and error behaviour:
//   ORB_SLAM2::ORBextractor  include/ORBextractor.h:46-114   (reference paths)
//   ORB_SLAM2::ORBmatcher    include/ORBmatcher.h:55-103     (all 11 methods + DescriptorDistance)
//   Frame::ComputeStereoMatches  src/Frame.cc:512-686
// cv::KeyPoint / cv::Mat / KeyFrame* / MapPoint* are replaced by layout-compatible PODs and flat arrays so
// that tests and tools build without OpenCV.  include/ORBextractor.h (extractor) and include/ORBmatcher.h +
// src/ORBmatcher_orbfe.cc (matcher) of this repo wrap these classes once more with the reference's exact
// signatures for a build that has OpenCV and the reference's own headers; those two are not compiled here.
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <map>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "orbfe.h"
#include "orbfe_initializer_replay.hpp"
#include "orbfe_pnp_replay.hpp"
#include "orbfe_sim3_replay.hpp"

namespace orbfe_cpp {

struct KeyPoint {  // == cv::KeyPoint, 28 bytes
  float x, y, size, angle, response;
  int32_t octave, class_id;
};
static_assert(sizeof(KeyPoint) == sizeof(orbfe_keypoint), "layout");

struct Image {  // minimal stand-in for a CV_8UC1 cv::Mat
  int cols = 0, rows = 0;
  std::vector<uint8_t> data;
  const uint8_t* ptr(int y) const { return data.data() + (size_t)y * cols; }
};

inline void check(int rc, const char* what) {
  if (rc < 0) throw std::runtime_error(std::string(what) + ": " + orbfe_last_error());
}

class ORBextractor {
 public:
  enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int iniThFAST, int minThFAST, int device = 0) {
    check(orbfe_extractor_create(nfeatures, scaleFactor, nlevels, iniThFAST, minThFAST, device, &h_), "ORBextractor");
  }
  ~ORBextractor() { orbfe_extractor_destroy(h_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // operator()(InputArray image, InputArray mask /*ignored*/, vector<KeyPoint>&, OutputArray descriptors)
  // Empty image: returns silently leaving the outputs untouched (src/ORBextractor.cc:1122-1123);
  // zero keypoints: descriptors released (:1145-1146).
  void operator()(const uint8_t* image, int width, int height, int stride, std::vector<KeyPoint>& keypoints,
                  std::vector<uint8_t>& descriptors) {
    if (!image || width <= 0 || height <= 0) return;
    int cap = orbfe_extractor_max_keypoints_for(h_, width, height);  // exact bound for this image size
    if (cap < orbfe_extractor_max_keypoints(h_)) cap = orbfe_extractor_max_keypoints(h_);
    keypoints.resize(cap);
    descriptors.resize((size_t)cap * 32);
    int n = 0;
    check(orbfe_extract(h_, image, width, height, stride, reinterpret_cast<orbfe_keypoint*>(keypoints.data()),
                        descriptors.data(), cap, &n), "ORBextractor::operator()");
    keypoints.resize(n);
    descriptors.resize((size_t)n * 32);
    w_ = width;
    h0_ = height;
    pyramidValid_ = false;
  }

  // The front end of the stereo Frame constructor in one call (src/Frame.cc:78-96: ExtractORB(0, imLeft) and
  // ExtractORB(1, imRight) on two threads, join, ComputeStereoMatches): both eyes through THIS handle, the stereo matcher on
  // the records still in HBM, one download.  mvuRight / mvDepth get keysLeft.size() entries (-1 = no stereo).
  void extractStereoFrame(const uint8_t* left, const uint8_t* right, int width, int height, int stride, float mbf, float mb,
                          std::vector<KeyPoint>& keysLeft, std::vector<uint8_t>& descLeft, std::vector<KeyPoint>& keysRight,
                          std::vector<uint8_t>& descRight, std::vector<float>& mvuRight, std::vector<float>& mvDepth) {
    if (!left || !right || width <= 0 || height <= 0) return;
    int cap = orbfe_extractor_max_keypoints_for(h_, width, height);
    if (cap < orbfe_extractor_max_keypoints(h_)) cap = orbfe_extractor_max_keypoints(h_);
    keysLeft.resize(cap); keysRight.resize(cap);
    descLeft.resize((size_t)cap * 32); descRight.resize((size_t)cap * 32);
    mvuRight.assign(cap, -1.0f); mvDepth.assign(cap, -1.0f);
    int nl = 0, nr = 0;
    check(orbfe_extract_stereo_frame(h_, left, right, width, height, stride, reinterpret_cast<orbfe_keypoint*>(keysLeft.data()),
                                     descLeft.data(), &nl, reinterpret_cast<orbfe_keypoint*>(keysRight.data()), descRight.data(),
                                     &nr, cap, mbf, mb, mvuRight.data(), mvDepth.data()), "ORBextractor::extractStereoFrame");
    keysLeft.resize(nl); keysRight.resize(nr);
    descLeft.resize((size_t)nl * 32); descRight.resize((size_t)nr * 32);
    mvuRight.resize(nl); mvDepth.resize(nl);
    w_ = width;
    h0_ = height;
    pyramidValid_ = false;
  }

  int GetLevels() { return orbfe_extractor_get_levels(h_); }
  float GetScaleFactor() { return orbfe_extractor_get_scale_factor(h_); }
  std::vector<float> GetScaleFactors() { return vec(orbfe_extractor_get_scale_factors); }
  std::vector<float> GetInverseScaleFactors() { return vec(orbfe_extractor_get_inverse_scale_factors); }
  std::vector<float> GetScaleSigmaSquares() { return vec(orbfe_extractor_get_scale_sigma_squares); }
  std::vector<float> GetInverseScaleSigmaSquares() { return vec(orbfe_extractor_get_inverse_scale_sigma_squares); }

  // The reference exposes `std::vector<cv::Mat> mvImagePyramid` (include/ORBextractor.h:86) that
  // Frame::ComputeStereoMatches reads.  Here the pyramid stays in HBM; this accessor copies it to
  // the host on first use after an extraction (the device stereo matcher never needs it).
  const std::vector<Image>& mvImagePyramid() {
    if (!pyramidValid_) {
      const int nl = GetLevels();
      pyr_.assign(nl, Image());
      for (int l = 0; l < nl && w_ > 0; l++) {
        Image& im = pyr_[l];
        check(orbfe_extractor_level_size(h_, w_, h0_, l, &im.cols, &im.rows), "level_size");
        im.data.resize((size_t)im.cols * im.rows);
        check(orbfe_extractor_get_pyramid_level(h_, 0, l, im.data.data(), im.cols), "get_pyramid_level");
      }
      pyramidValid_ = true;
    }
    return pyr_;
  }

  orbfe_extractor* handle() { return h_; }

 private:
  template <typename F>
  std::vector<float> vec(F f) {
    std::vector<float> v(GetLevels());
    check(f(h_, v.data()), "getter");
    return v;
  }
  orbfe_extractor* h_ = nullptr;
  int w_ = 0, h0_ = 0;
  bool pyramidValid_ = false;
  std::vector<Image> pyr_;
};

// DBoW2::FeatureVector (std::map<NodeId, std::vector<unsigned>>) -> CSR view for the C-ABI
struct FeatureVectorCSR {
  std::vector<uint32_t> node_ids, indices;
  std::vector<int32_t> offsets;
  orbfe_featvec c{};
  template <typename Map>
  explicit FeatureVectorCSR(const Map& fv) {
    offsets.push_back(0);
    for (const auto& kv : fv) {
      node_ids.push_back((uint32_t)kv.first);
      for (unsigned i : kv.second) indices.push_back(i);
      offsets.push_back((int32_t)indices.size());
    }
    c.n_nodes = (int32_t)node_ids.size();
    c.node_ids = node_ids.data();
    c.offsets = offsets.data();
    c.indices = indices.data();
  }
};

// The arrays of a Frame / KeyFrame the projection searches read (include/Frame.h:120-190), split out of
// std::vector<cv::KeyPoint> mvKeysUn once per frame; owns the storage behind an orbfe_frame_view.
class FrameArrays {
 public:
  // bounds = mnMinX, mnMaxX, mnMinY, mnMaxY (src/Frame.cc:697-728); mvuRight may be empty (monocular)
  FrameArrays(const std::vector<KeyPoint>& mvKeysUn, const std::vector<uint8_t>& mDescriptors, float mnMinX,
              float mnMaxX, float mnMinY, float mnMaxY, const std::vector<float>& mvuRight = std::vector<float>())
      : desc(mDescriptors), uRight(mvuRight) {
    const size_t n = mvKeysUn.size();
    x.resize(n); y.resize(n); angle.resize(n); octave.resize(n);
    for (size_t i = 0; i < n; i++) {
      x[i] = mvKeysUn[i].x; y[i] = mvKeysUn[i].y; angle[i] = mvKeysUn[i].angle; octave[i] = mvKeysUn[i].octave;
    }
    c.n = (int32_t)n;
    c.x = x.data(); c.y = y.data(); c.octave = octave.data(); c.angle = angle.data();
    c.u_right = uRight.empty() ? nullptr : uRight.data();
    c.desc = desc.data();
    c.min_x = mnMinX; c.max_x = mnMaxX; c.min_y = mnMinY; c.max_y = mnMaxY;
    c.resident = nullptr;
  }
  ~FrameArrays() { if (resident_) orbfe_frame_release(resident_); }
  FrameArrays(const FrameArrays&) = delete;
  FrameArrays& operator=(const FrameArrays&) = delete;
  int N() const { return c.n; }

  // Move this frame's operands to the device ONCE (keypoint arrays, descriptors, the 64 x 48 grid, and -- for the
  // FeatureVector searches -- mFeatVec's index list): every later search on this object uploads nothing of the frame.
  // Call it where the reference fills the object for good: at the end of the Frame constructor / in
  // KeyFrame::ComputeBoW (src/KeyFrame.cc:64-73).  A KeyFrame is matched against 10-20 neighbours per insertion.
  void makeResident(const FeatureVectorCSR* mFeatVec = nullptr, int device = 0) {
    if (resident_) { orbfe_frame_release(resident_); resident_ = nullptr; c.resident = nullptr; }
    check(orbfe_frame_upload(device, &c, mFeatVec ? &mFeatVec->c : nullptr, &resident_), "FrameArrays::makeResident");
    c.resident = resident_;
  }
  // The same from the extractor's OWN device records -- Frame::Frame is ExtractORB -> UndistortKeyPoints ->
  // ComputeStereoMatches -> AssignFeaturesToGrid (src/Frame.cc:61-117): the keypoints and descriptors operator() just
  // returned are still in HBM, so only mvuRight (and, for cameras with distortion, the undistorted positions:
  // undistorted = true) travel.  `e` = the extractor whose last operator() produced this frame's keypoints.
  void makeResidentFromExtractor(const orbfe_extractor* e, bool undistorted = false, const FeatureVectorCSR* mFeatVec = nullptr) {
    if (resident_) { orbfe_frame_release(resident_); resident_ = nullptr; c.resident = nullptr; }
    check(orbfe_frame_from_extractor(const_cast<orbfe_extractor*>(e), 0, &c, mFeatVec ? &mFeatVec->c : nullptr,
                                     undistorted ? ORBFE_FRAME_XY_FROM_VIEW : 0, &resident_), "FrameArrays::makeResidentFromExtractor");
    c.resident = resident_;
  }
  // Frame::ComputeBoW (src/Frame.cc:433-440) runs after the constructor: attach mFeatVec to the resident frame
  void setFeatVec(const FeatureVectorCSR& mFeatVec) { check(orbfe_frame_set_featvec(resident_, &mFeatVec.c), "FrameArrays::setFeatVec"); }
  // returns once the resident build has completed on the device (device arrays a build from them read may be reused)
  void synchronize() const { check(orbfe_frame_synchronize(resident_), "FrameArrays::synchronize"); }
  const orbfe_frame* resident() const { return resident_; }

  // vector<size_t> Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) const
  std::vector<size_t> GetFeaturesInArea(float qx, float qy, float r, int minLevel = -1, int maxLevel = -1,
                                        int device = 0) const {
    int32_t count = 0;
    std::vector<int32_t> idx(64);
    for (;;) {
      const int rc = orbfe_features_in_area(device, &c, 1, &qx, &qy, &r, &minLevel, &maxLevel, (int)idx.size(), &count,
                                            idx.data());
      if (rc == ORBFE_ERR_CAPACITY) { idx.resize(count); continue; }
      check(rc, "GetFeaturesInArea");
      break;
    }
    return std::vector<size_t>(idx.begin(), idx.begin() + count);
  }

  std::vector<float> x, y, angle;
  std::vector<int32_t> octave;
  std::vector<uint8_t> desc;
  std::vector<float> uRight;
  orbfe_frame_view c;

 private:
  orbfe_frame* resident_ = nullptr;
};

// What LocalMapping::CreateNewMapPoints reads of a key frame besides its keypoints (orbfe_keyframe_camera); owns the arrays.
// Tcw: the 3 x 4 [Rcw | tcw] (GetRotation / GetTranslation), row-major; Ow = GetCameraCenter(); mvDepth empty: monocular;
// mvKeysX / mvKeysY (the raw positions UnprojectStereo reads, src/KeyFrame.cc:663-664) empty: the frame's own mvKeysUn.
struct KeyFrameCamera {
  KeyFrameCamera(const float Tcw[12], const float Ow[3], float fx, float fy, float cx, float cy, float invfx, float invfy,
                 float mb, float mbf, const std::vector<float>& mvDepth = std::vector<float>(),
                 const std::vector<float>& mvKeysX = std::vector<float>(), const std::vector<float>& mvKeysY = std::vector<float>())
      : depth(mvDepth), xRaw(mvKeysX), yRaw(mvKeysY) {
    std::memcpy(c_.Tcw, Tcw, sizeof c_.Tcw);
    std::memcpy(c_.Ow, Ow, sizeof c_.Ow);
    c_.fx = fx; c_.fy = fy; c_.cx = cx; c_.cy = cy; c_.invfx = invfx; c_.invfy = invfy; c_.mb = mb; c_.mbf = mbf;
  }
  // (pointers are taken at the call: the object may have been copied or moved since it was made)
  orbfe_keyframe_camera c() const {
    orbfe_keyframe_camera r = c_;
    r.depth = depth.empty() ? nullptr : depth.data();
    r.x_raw = xRaw.empty() ? nullptr : xRaw.data();
    r.y_raw = yRaw.empty() ? nullptr : yRaw.data();
    return r;
  }
  std::vector<float> depth, xRaw, yRaw;

 private:
  orbfe_keyframe_camera c_ = {};
};

class ORBmatcher {
 public:
  static const int TH_LOW = 50;
  static const int TH_HIGH = 100;
  static const int HISTO_LENGTH = 30;

  ORBmatcher(float nnratio = 0.6f, bool checkOri = true, int device = 0)
      : mfNNratio(nnratio), mbCheckOrientation(checkOri), device_(device) {}

  // static int DescriptorDistance(const cv::Mat& a, const cv::Mat& b)
  static int DescriptorDistance(const uint8_t* a, const uint8_t* b, int device = 0) {
    int32_t d = 0;
    check(orbfe_descriptor_distance(device, a, b, 1, &d), "DescriptorDistance");
    return d;
  }

  // int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches):
  // matchF[j] = KF feature whose MapPoint goes to frame feature j (or -1).
  int SearchByBoW(const uint8_t* descKF, const uint8_t* hasMapPointKF, const float* angleKF, int nKF,
                  const FeatureVectorCSR& fvKF, const uint8_t* descF, const float* angleF, int nF,
                  const FeatureVectorCSR& fvF, std::vector<int32_t>& matchF) {
    matchF.assign(nF, -1);
    int rc = orbfe_search_by_bow(device_, descKF, hasMapPointKF, angleKF, nKF, &fvKF.c, descF, angleF, nF, &fvF.c,
                                 mfNNratio, mbCheckOrientation, matchF.data());
    check(rc, "SearchByBoW");
    return rc;
  }
  // int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)
  int SearchByBoW(const uint8_t* desc1, const uint8_t* hasMp1, const float* angle1, int n1,
                  const FeatureVectorCSR& fv1, const uint8_t* desc2, const uint8_t* hasMp2, const float* angle2,
                  int n2, const FeatureVectorCSR& fv2, std::vector<int32_t>& match12) {
    match12.assign(n1, -1);
    int rc = orbfe_search_by_bow_kf(device_, desc1, hasMp1, angle1, n1, &fv1.c, desc2, hasMp2, angle2, n2, &fv2.c,
                                    mfNNratio, mbCheckOrientation, match12.data());
    check(rc, "SearchByBoW(KF,KF)");
    return rc;
  }

  // int SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, const float th = 3):
  // the per-point fields are what Frame::isInFrustum stored on each MapPoint; match[idx] = point or -1.
  int SearchByProjection(const FrameArrays& F, const std::vector<float>& mvScaleFactors,
                         const std::vector<uint8_t>& mbTrackInView, const std::vector<int32_t>& mnTrackScaleLevel,
                         const std::vector<float>& mTrackViewCos, const std::vector<float>& mTrackProjX,
                         const std::vector<float>& mTrackProjY, const std::vector<float>& mTrackProjXR,
                         const std::vector<uint8_t>& mpDescriptors, const std::vector<uint8_t>& frameHasObservedPoint,
                         std::vector<int32_t>& match, float th = 3.0f) {
    match.assign(F.N(), -1);
    int32_t n = 0;
    check(orbfe_search_by_projection(device_, &F.c, mvScaleFactors.data(), (int)mvScaleFactors.size(),
                                     frameHasObservedPoint.empty() ? nullptr : frameHasObservedPoint.data(),
                                     (int)mbTrackInView.size(), mbTrackInView.data(), mnTrackScaleLevel.data(),
                                     mTrackViewCos.data(), mTrackProjX.data(), mTrackProjY.data(),
                                     mTrackProjXR.empty() ? nullptr : mTrackProjXR.data(), mpDescriptors.data(), nullptr,
                                     th, mfNNratio, match.data(), &n),
          "SearchByProjection(Frame,MapPoints)");
    return n;
  }

  // int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, const float th, const bool bMono)
  // after the projection loop prologue (src/ORBmatcher.cc:1525-1541); mode 0/1/2 = normal/bForward/bBackward.
  int SearchByProjection(const FrameArrays& CurrentFrame, const std::vector<float>& mvScaleFactors, float mbf,
                         const std::vector<uint8_t>& valid, const std::vector<float>& u, const std::vector<float>& v,
                         const std::vector<float>& invzc, const std::vector<int32_t>& lastOctave,
                         const std::vector<float>& lastAngle, const std::vector<uint8_t>& mpDescriptors, int mode,
                         float th, std::vector<int32_t>& matchCur,
                         const std::vector<uint8_t>& obsPositive = std::vector<uint8_t>(),
                         const std::vector<uint8_t>& curBlocked = std::vector<uint8_t>()) {
    matchCur.assign(CurrentFrame.N(), -1);
    int32_t n = 0;
    check(orbfe_search_by_projection_last_frame(device_, &CurrentFrame.c, mvScaleFactors.data(),
                                                (int)mvScaleFactors.size(), mbf, (int)valid.size(), valid.data(),
                                                u.data(), v.data(), invzc.empty() ? nullptr : invzc.data(),
                                                lastOctave.data(), lastAngle.data(), mpDescriptors.data(),
                                                obsPositive.empty() ? nullptr : obsPositive.data(),
                                                curBlocked.empty() ? nullptr : curBlocked.data(), mode,
                                                th, mbCheckOrientation, matchCur.data(), &n),
          "SearchByProjection(Frame,Frame)");
    return n;
  }

  // int SearchForInitialization(Frame& F1, Frame& F2, vector<cv::Point2f>& vbPrevMatched,
  //                             vector<int>& vnMatches12, int windowSize = 10)
  int SearchForInitialization(const FrameArrays& F1, const FrameArrays& F2, std::vector<float>& prevX,
                              std::vector<float>& prevY, std::vector<int32_t>& vnMatches12, int windowSize = 10) {
    vnMatches12.assign(F1.N(), -1);
    int32_t n = 0;
    check(orbfe_search_for_initialization(device_, &F1.c, &F2.c, prevX.data(), prevY.data(), windowSize, mfNNratio,
                                          mbCheckOrientation, vnMatches12.data(), &n),
          "SearchForInitialization");
    return n;
  }

  // int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, cv::Mat F12,
  //                            vector<pair<size_t,size_t>>& vMatchedPairs, const bool bOnlyStereo)
  // (src/ORBmatcher.cc:754-928).  KF1 / KF2 carry mvKeysUn + mvuRight; hasMp = "GetMapPoint(idx) != NULL";
  // F12 row-major 3x3; (ex, ey) = the epipole of :766-769; mvScaleFactors2 / mvLevelSigma2_2 of pKF2.
  int SearchForTriangulation(const FrameArrays& KF1, const std::vector<uint8_t>& hasMp1, const FeatureVectorCSR& fv1,
                             const FrameArrays& KF2, const std::vector<uint8_t>& hasMp2, const FeatureVectorCSR& fv2,
                             const float F12[9], float ex, float ey, const std::vector<float>& mvScaleFactors2,
                             const std::vector<float>& mvLevelSigma2_2, std::vector<std::pair<size_t, size_t> >& vMatchedPairs,
                             bool bOnlyStereo) {
    const int n1 = KF1.N(), n2 = KF2.N();
    std::vector<uint8_t> st1(n1, 0), st2(n2, 0);  // bStereo1 = mvuRight[idx] >= 0 (:806, :830)
    for (int i = 0; i < n1 && !KF1.uRight.empty(); i++) st1[i] = KF1.uRight[i] >= 0;
    for (int i = 0; i < n2 && !KF2.uRight.empty(); i++) st2[i] = KF2.uRight[i] >= 0;
    std::vector<int32_t> match12(n1 > 0 ? n1 : 1, -1);
    const int rc = orbfe_search_for_triangulation(
        device_, KF1.desc.data(), hasMp1.data(), KF1.x.data(), KF1.y.data(), KF1.angle.data(), st1.data(), n1, &fv1.c,
        KF2.desc.data(), hasMp2.data(), KF2.x.data(), KF2.y.data(), KF2.angle.data(), KF2.octave.data(), st2.data(), n2,
        &fv2.c, F12, ex, ey, mvScaleFactors2.data(), mvLevelSigma2_2.data(), (int)mvScaleFactors2.size(), bOnlyStereo,
        mbCheckOrientation, match12.data());
    check(rc, "SearchForTriangulation");
    vMatchedPairs.clear();
    vMatchedPairs.reserve(rc);
    for (int i = 0; i < n1; i++)  // :920-925: ascending idx1
      if (match12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)match12[i]));
    return rc;
  }

  // The loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:283-315) in ONE call: SearchForTriangulation of
  // pKF1 against every neighbour.  All frames resident (makeResident with their mFeatVec).  F12s[k] / epipoles[k] as the
  // single-pair form takes them; vMatchedPairs[k] = the pairs of neighbour k (ascending idx1).
  void SearchForTriangulationMulti(const FrameArrays& KF1, const std::vector<uint8_t>& hasMp1,
                                   const std::vector<const FrameArrays*>& neighbours,
                                   const std::vector<const std::vector<uint8_t>*>& hasMp2, const std::vector<float>& F12s /* 9 per neighbour */,
                                   const std::vector<float>& ex, const std::vector<float>& ey,
                                   const std::vector<float>& mvScaleFactors2, const std::vector<float>& mvLevelSigma2_2,
                                   std::vector<std::vector<std::pair<size_t, size_t> > >& vMatchedPairs, bool bOnlyStereo) {
    const int K = (int)neighbours.size(), n1 = KF1.N();
    std::vector<const orbfe_frame*> fr(K > 0 ? K : 1, nullptr);
    std::vector<const uint8_t*> mk(K > 0 ? K : 1, nullptr);
    for (int k = 0; k < K; k++) { fr[k] = neighbours[k]->resident(); mk[k] = hasMp2[k]->data(); }
    std::vector<int32_t> match((size_t)(K > 0 ? K : 1) * (n1 > 0 ? n1 : 1), -1), cnt(K > 0 ? K : 1, 0);
    check(orbfe_search_for_triangulation_multi(KF1.resident(), hasMp1.data(), K, fr.data(), mk.data(), F12s.data(), ex.data(),
                                               ey.data(), mvScaleFactors2.data(), mvLevelSigma2_2.data(),
                                               (int)mvScaleFactors2.size(), bOnlyStereo, mbCheckOrientation, match.data(), cnt.data()),
          "SearchForTriangulationMulti");
    vMatchedPairs.assign(K, std::vector<std::pair<size_t, size_t> >());
    for (int k = 0; k < K; k++)
      for (int i = 0; i < n1; i++)
        if (match[(size_t)k * n1 + i] >= 0) vMatchedPairs[k].push_back(std::make_pair((size_t)i, (size_t)match[(size_t)k * n1 + i]));
  }

  // The per-pair loop of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:331-501) for every pair
  // SearchForTriangulationMulti matched, in ONE call (orbfe_triangulate_matches_multi): match12[k * n1 + i1] = keypoint of
  // neighbour k or -1; x3d [3 per slot], status (ORBFE_TRI_*) and winner as include/orbfe.h describes them; nCreated[k].
  // Replay the neighbours in order and keep, for keypoint i1, only the pair with status CREATED and winner[i1] == k.
  // Frames may be resident or not.
  void TriangulateMatchesMulti(const FrameArrays& KF1, const KeyFrameCamera& cam1, const std::vector<const FrameArrays*>& neighbours,
                               const std::vector<const KeyFrameCamera*>& cams, const std::vector<int32_t>& match12,
                               const std::vector<float>& mvScaleFactors, const std::vector<float>& mvLevelSigma2, float ratioFactor,
                               std::vector<float>& x3d, std::vector<uint8_t>& status, std::vector<int32_t>& nCreated,
                               std::vector<int32_t>& winner) {
    const int K = (int)neighbours.size(), n1 = KF1.N();
    std::vector<const orbfe_frame_view*> views(K > 0 ? K : 1, nullptr);
    std::vector<orbfe_keyframe_camera> cc(K > 0 ? K : 1);
    for (int k = 0; k < K; k++) { views[k] = &neighbours[k]->c; cc[k] = cams[k]->c(); }
    const orbfe_keyframe_camera c1 = cam1.c();
    const size_t slots = (size_t)K * n1;
    x3d.assign(slots * 3, 0.0f); status.assign(slots, 0); nCreated.assign(K, 0); winner.assign(n1, -1);
    std::vector<float> xb(slots * 3 + 1);
    std::vector<uint8_t> sb(slots + 1);
    std::vector<int32_t> nb((size_t)K + 1), wb((size_t)n1 + 1);
    check(orbfe_triangulate_matches_multi(device_, &KF1.c, &c1, K, views.data(), cc.data(), match12.data(), mvScaleFactors.data(),
                                          mvLevelSigma2.data(), (int)mvScaleFactors.size(), ratioFactor, xb.data(), sb.data(),
                                          nb.data(), wb.data()),
          "TriangulateMatchesMulti");
    std::copy(xb.begin(), xb.begin() + slots * 3, x3d.begin()); std::copy(sb.begin(), sb.begin() + slots, status.begin());
    std::copy(nb.begin(), nb.begin() + K, nCreated.begin()); std::copy(wb.begin(), wb.begin() + n1, winner.begin());
  }
  // one neighbour: match12 [n1]; returns the number of points created
  int TriangulateMatches(const FrameArrays& KF1, const KeyFrameCamera& cam1, const FrameArrays& KF2, const KeyFrameCamera& cam2,
                         const std::vector<int32_t>& match12, const std::vector<float>& mvScaleFactors,
                         const std::vector<float>& mvLevelSigma2, float ratioFactor, std::vector<float>& x3d,
                         std::vector<uint8_t>& status) {
    const int n1 = KF1.N();
    const orbfe_keyframe_camera c1 = cam1.c(), c2 = cam2.c();
    std::vector<float> xb((size_t)n1 * 3 + 1);
    std::vector<uint8_t> sb((size_t)n1 + 1);
    int32_t created = 0;
    check(orbfe_triangulate_matches(device_, &KF1.c, &c1, &KF2.c, &c2, match12.data(), mvScaleFactors.data(), mvLevelSigma2.data(),
                                    (int)mvScaleFactors.size(), ratioFactor, xb.data(), sb.data(), &created),
          "TriangulateMatches");
    x3d.assign(xb.begin(), xb.begin() + (size_t)n1 * 3); status.assign(sb.begin(), sb.begin() + n1);
    return created;
  }
  // Where the created pairs become map points (orbfe_triangulated_points_select; src/LocalMapping.cc:484-500), on the arrays
  // TriangulateMatchesMulti returns: who is created and in what order (ascending (k, i1), the first neighbour that succeeds
  // has the keypoint), the position, the two-observation normal and range, and which key frame's descriptor wins (descFrom
  // 0: key frame 1's row i1, 1: the neighbour's row i2 -- the smaller mnId).  centre1 [3], centre2 [3 per neighbour]; octave1 =
  // key frame 1's octaves.  Host code: needs no device.  More created points than `capacity` throws.
  struct TriangulatedPoints {
    std::vector<int32_t> k, i1, i2;
    std::vector<float> pos, normal, minDist, maxDist;  // pos / normal: 3 per point
    std::vector<uint8_t> descFrom;
  };
  static TriangulatedPoints TriangulatedPointsSelect(int n1, const std::vector<int32_t>& match12, const std::vector<uint8_t>& status,
                                                     const std::vector<float>& x3d, int64_t kf1Id, const std::vector<int64_t>& kf2Id,
                                                     const std::vector<float>& centre1, const std::vector<float>& centre2,
                                                     const std::vector<int32_t>& octave1, const std::vector<float>& mvScaleFactors,
                                                     int capacity) {
    const int K = (int)kf2Id.size();
    if (match12.size() != (size_t)K * n1 || status.size() != match12.size() || x3d.size() != 3 * match12.size() || centre1.size() != 3 ||
        centre2.size() != 3 * (size_t)K || octave1.size() != (size_t)n1)
      throw std::invalid_argument("ORBmatcher::TriangulatedPointsSelect: array sizes do not fit n1 and the neighbours");
    const size_t cap = (size_t)(capacity > 0 ? capacity : 0);
    TriangulatedPoints out;
    out.k.assign(cap + 1, 0); out.i1.assign(cap + 1, 0); out.i2.assign(cap + 1, 0);
    out.pos.assign(3 * cap + 1, 0.0f); out.normal.assign(3 * cap + 1, 0.0f); out.minDist.assign(cap + 1, 0.0f); out.maxDist.assign(cap + 1, 0.0f);
    out.descFrom.assign(cap + 1, 0);
    int32_t created = 0;
    check(orbfe_triangulated_points_select(n1, K, match12.data(), status.data(), x3d.data(), kf1Id, kf2Id.data(), centre1.data(),
                                           centre2.data(), octave1.data(), mvScaleFactors.data(), (int)mvScaleFactors.size(), capacity,
                                           out.k.data(), out.i1.data(), out.i2.data(), out.pos.data(), out.normal.data(), out.minDist.data(),
                                           out.maxDist.data(), out.descFrom.data(), &created),
          "TriangulatedPointsSelect");
    const size_t m = (size_t)created;
    out.k.resize(m); out.i1.resize(m); out.i2.resize(m); out.pos.resize(3 * m); out.normal.resize(3 * m); out.minDist.resize(m);
    out.maxDist.resize(m); out.descFrom.resize(m);
    return out;
  }

  // The loop of Tracking::Relocalization (src/Tracking.cc:1478-1498) in ONE call: SearchByBoW(pKF_k, mCurrentFrame,
  // vvpMapPointMatches[k]) for every candidate key frame.  All frames resident with their mFeatVec.  vnMatches[k][i2] =
  // feature of key frame k whose MapPoint goes to feature i2 of the frame, or -1; returns the counts.
  std::vector<int> SearchByBoWMulti(const std::vector<const FrameArrays*>& vpCandidateKFs,
                                    const std::vector<const std::vector<uint8_t>*>& hasMp, const FrameArrays& F,
                                    std::vector<std::vector<int32_t> >& vnMatches) {
    const int K = (int)vpCandidateKFs.size(), n = F.N();
    std::vector<const orbfe_frame*> fr(K > 0 ? K : 1, nullptr);
    std::vector<const uint8_t*> mk(K > 0 ? K : 1, nullptr);
    for (int k = 0; k < K; k++) { fr[k] = vpCandidateKFs[k]->resident(); mk[k] = hasMp[k]->data(); }
    std::vector<int32_t> match((size_t)(K > 0 ? K : 1) * (n > 0 ? n : 1), -1), cnt(K > 0 ? K : 1, 0);
    check(orbfe_search_by_bow_multi(K, fr.data(), mk.data(), F.resident(), mfNNratio, mbCheckOrientation, match.data(), cnt.data()),
          "SearchByBoWMulti");
    vnMatches.assign(K, std::vector<int32_t>());
    for (int k = 0; k < K; k++) vnMatches[k].assign(match.begin() + (size_t)k * n, match.begin() + (size_t)(k + 1) * n);
    return std::vector<int>(cnt.begin(), cnt.begin() + K);
  }
  // The loop of LoopClosing::ComputeSim3 (src/LoopClosing.cc:294-321): SearchByBoW(mpCurrentKF, pKF_k, vvpMapPointMatches[k]).
  // vnMatches12[k][i1] = feature of candidate k matched to feature i1 of the current key frame, or -1.
  std::vector<int> SearchByBoWMulti(const FrameArrays& KF1, const std::vector<uint8_t>& hasMp1,
                                    const std::vector<const FrameArrays*>& vpCandidateKFs,
                                    const std::vector<const std::vector<uint8_t>*>& hasMp2,
                                    std::vector<std::vector<int32_t> >& vnMatches12) {
    const int K = (int)vpCandidateKFs.size(), n = KF1.N();
    std::vector<const orbfe_frame*> fr(K > 0 ? K : 1, nullptr);
    std::vector<const uint8_t*> mk(K > 0 ? K : 1, nullptr);
    for (int k = 0; k < K; k++) { fr[k] = vpCandidateKFs[k]->resident(); mk[k] = hasMp2[k]->data(); }
    std::vector<int32_t> match((size_t)(K > 0 ? K : 1) * (n > 0 ? n : 1), -1), cnt(K > 0 ? K : 1, 0);
    check(orbfe_search_by_bow_kf_multi(KF1.resident(), hasMp1.data(), K, fr.data(), mk.data(), mfNNratio, mbCheckOrientation,
                                       match.data(), cnt.data()),
          "SearchByBoWMulti(KF,KF)");
    vnMatches12.assign(K, std::vector<int32_t>());
    for (int k = 0; k < K; k++) vnMatches12[k].assign(match.begin() + (size_t)k * n, match.begin() + (size_t)(k + 1) * n);
    return std::vector<int>(cnt.begin(), cnt.begin() + K);
  }

  // SearchByProjection(mCurrentFrame, vpCandidateKFs[k], sFound, th_k, ORBdist_k) (src/Tracking.cc:1577,1595) for several
  // candidates in ONE call; one ProjectedKeyFrame per candidate = the caller's projection prologue (:1657-1700).
  struct ProjectedKeyFrame {
    std::vector<uint8_t> valid, mpDescriptors, curHasMapPoint /* may be empty */;
    std::vector<float> u, v, kfAngle;
    std::vector<int32_t> level;
    float th; int ORBdist;
  };
  std::vector<int> SearchByProjectionMulti(const FrameArrays& CurrentFrame, const std::vector<float>& mvScaleFactors,
                                           const std::vector<ProjectedKeyFrame>& cands, std::vector<std::vector<int32_t> >& matchCur) {
    const int K = (int)cands.size(), n = CurrentFrame.N(), K1 = K > 0 ? K : 1;
    std::vector<const uint8_t*> blk(K1, nullptr), va(K1, nullptr), md(K1, nullptr);
    std::vector<const float*> u(K1, nullptr), v(K1, nullptr), ka(K1, nullptr);
    std::vector<const int32_t*> lv(K1, nullptr);
    std::vector<int32_t> nk(K1, 0), od(K1, 0), match((size_t)K1 * (n > 0 ? n : 1), -1), cnt(K1, 0);
    std::vector<float> th(K1, 0.f);
    for (int k = 0; k < K; k++) {
      const ProjectedKeyFrame& c = cands[k];
      blk[k] = c.curHasMapPoint.empty() ? nullptr : c.curHasMapPoint.data();
      va[k] = c.valid.data(); md[k] = c.mpDescriptors.data(); u[k] = c.u.data(); v[k] = c.v.data(); ka[k] = c.kfAngle.data();
      lv[k] = c.level.data(); nk[k] = (int32_t)c.valid.size(); od[k] = c.ORBdist; th[k] = c.th;
    }
    check(orbfe_search_by_projection_keyframe_multi(device_, &CurrentFrame.c, mvScaleFactors.data(), (int)mvScaleFactors.size(), K,
                                                    blk.data(), nk.data(), va.data(), u.data(), v.data(), lv.data(), ka.data(), md.data(),
                                                    th.data(), od.data(), mbCheckOrientation, match.data(), cnt.data()),
          "SearchByProjectionMulti");
    matchCur.assign(K, std::vector<int32_t>());
    for (int k = 0; k < K; k++) matchCur[k].assign(match.begin() + (size_t)k * n, match.begin() + (size_t)(k + 1) * n);
    return std::vector<int>(cnt.begin(), cnt.begin() + K);
  }

  // The per-point search of Fuse for the SAME map points against K key frames in one call (LocalMapping::SearchInNeighbors,
  // src/LocalMapping.cc:542-549): per-key-frame arrays are [k * n + i] (the caller's projection prologue per key frame,
  // src/ORBmatcher.cc:960-1020); bestIdx[k * n + i] = keypoint of key frame k chosen for point i, or -1.
  void FuseSearchMulti(const std::vector<const FrameArrays*>& KFs, const std::vector<float>& mvScaleFactors,
                       const std::vector<float>& mvInvLevelSigma2, int nPoints, const std::vector<uint8_t>& valid,
                       const std::vector<float>& u, const std::vector<float>& v, const std::vector<float>& ur,
                       const std::vector<int32_t>& level, const std::vector<uint8_t>& mpDescriptors, float th,
                       std::vector<int32_t>& bestIdx) {
    const int K = (int)KFs.size();
    std::vector<const orbfe_frame_view*> views(K > 0 ? K : 1, nullptr);
    for (int k = 0; k < K; k++) views[k] = &KFs[k]->c;
    bestIdx.assign((size_t)K * nPoints, -1);
    check(orbfe_fuse_search_multi(device_, K, views.data(), mvScaleFactors.data(), mvInvLevelSigma2.data(),
                                  (int)mvScaleFactors.size(), nPoints, valid.data(), u.data(), v.data(),
                                  ur.empty() ? nullptr : ur.data(), level.data(), mpDescriptors.data(), th, 1, bestIdx.data()),
          "FuseSearchMulti");
  }

  // int SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, const set<MapPoint*>& sAlreadyFound, const float th,
  //                        const int ORBdist) (src/ORBmatcher.cc:1641-1775, relocalisation) after the caller's
  // projection prologue (:1657-1700): valid[i] = pKF's map point i exists, is good, not in sAlreadyFound, projects
  // inside the image and its distance range; level = PredictScale; kfAngle = pKF->mvKeysUn[i].angle;
  // curHasMapPoint[i2] = CurrentFrame.mvpMapPoints[i2] != NULL (may be empty).  matchCur[i2] = index i or -1.
  int SearchByProjection(const FrameArrays& CurrentFrame, const std::vector<float>& mvScaleFactors,
                         const std::vector<uint8_t>& curHasMapPoint, const std::vector<uint8_t>& valid,
                         const std::vector<float>& u, const std::vector<float>& v, const std::vector<int32_t>& level,
                         const std::vector<float>& kfAngle, const std::vector<uint8_t>& mpDescriptors, float th,
                         int ORBdist, std::vector<int32_t>& matchCur) {
    matchCur.assign(CurrentFrame.N(), -1);
    int32_t n = 0;
    check(orbfe_search_by_projection_keyframe(device_, &CurrentFrame.c, mvScaleFactors.data(), (int)mvScaleFactors.size(),
                                              curHasMapPoint.empty() ? nullptr : curHasMapPoint.data(), (int)valid.size(),
                                              valid.data(), u.data(), v.data(), level.data(), kfAngle.data(),
                                              mpDescriptors.data(), th, ORBdist, mbCheckOrientation, matchCur.data(), &n),
          "SearchByProjection(Frame,KeyFrame)");
    return n;
  }

  // int SearchByProjection(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints,
  //                        vector<MapPoint*>& vpMatched, int th) (src/ORBmatcher.cc:335-449, loop closing) after the
  // caller's Sim3 projection (:355-400): valid[i] = point i is good, not already in vpMatched, in front of the
  // camera, inside the image, its distance range and viewing cone.  alreadyMatched[idx] = vpMatched[idx] != NULL
  // (may be empty).  match[idx] = point newly matched to keypoint idx, or -1.
  int SearchByProjection(const FrameArrays& KF, const std::vector<float>& mvScaleFactors,
                         const std::vector<uint8_t>& alreadyMatched, const std::vector<uint8_t>& valid,
                         const std::vector<float>& u, const std::vector<float>& v, const std::vector<int32_t>& level,
                         const std::vector<uint8_t>& mpDescriptors, int th, std::vector<int32_t>& match) {
    match.assign(KF.N(), -1);
    int32_t n = 0;
    check(orbfe_search_by_projection_sim3(device_, &KF.c, mvScaleFactors.data(), (int)mvScaleFactors.size(),
                                          alreadyMatched.empty() ? nullptr : alreadyMatched.data(), (int)valid.size(),
                                          valid.data(), u.data(), v.data(), level.data(), mpDescriptors.data(), (float)th,
                                          match.data(), &n),
          "SearchByProjection(KeyFrame,Scw)");
    return n;
  }

  // The search inside int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th = 3.0)
  // (src/ORBmatcher.cc:940-1110): per map point, after the caller's projection (:960-1020, valid / u / v / ur /
  // PredictScale level), bestIdx[i] = the keypoint of pKF to fuse with, or -1.  Replace / AddObservation on a hit
  // (:1088-1106) is map bookkeeping and stays with the caller.  ur is read for stereo keypoints only.
  void Fuse(const FrameArrays& KF, const std::vector<float>& mvScaleFactors, const std::vector<float>& mvInvLevelSigma2,
            const std::vector<uint8_t>& valid, const std::vector<float>& u, const std::vector<float>& v,
            const std::vector<float>& ur, const std::vector<int32_t>& level, const std::vector<uint8_t>& mpDescriptors,
            std::vector<int32_t>& bestIdx, float th = 3.0f) {
    bestIdx.assign(valid.size(), -1);
    check(orbfe_fuse_search(device_, &KF.c, mvScaleFactors.data(), mvInvLevelSigma2.data(), (int)mvScaleFactors.size(),
                            (int)valid.size(), valid.data(), u.data(), v.data(), ur.empty() ? nullptr : ur.data(),
                            level.data(), mpDescriptors.data(), th, 1, bestIdx.data()),
          "Fuse");
  }
  // The search inside int Fuse(KeyFrame* pKF, cv::Mat Scw, const vector<MapPoint*>& vpPoints, float th,
  //                            vector<MapPoint*>& vpReplacePoint) (src/ORBmatcher.cc:1112-1249): no chi2 gate.
  void Fuse(const FrameArrays& KF, const std::vector<float>& mvScaleFactors, const std::vector<uint8_t>& valid,
            const std::vector<float>& u, const std::vector<float>& v, const std::vector<int32_t>& level,
            const std::vector<uint8_t>& mpDescriptors, float th, std::vector<int32_t>& bestIdx) {
    bestIdx.assign(valid.size(), -1);
    check(orbfe_fuse_search(device_, &KF.c, mvScaleFactors.data(), nullptr, (int)mvScaleFactors.size(),
                            (int)valid.size(), valid.data(), u.data(), v.data(), nullptr, level.data(),
                            mpDescriptors.data(), th, 0, bestIdx.data()),
          "Fuse(Scw)");
  }

  // int SearchBySim3(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12, const float& s12,
  //                  const cv::Mat& R12, const cv::Mat& t12, const float th) (src/ORBmatcher.cc:1251-1482) after the
  // caller's two projection loops: valid1[i1] = map point of KF1 keypoint i1 is good, not matched yet, projects
  // into KF2 (u1, v1) inside the image and its distance range, level1 = PredictScale(pKF2), desc1 = its
  // descriptor; the "2" arrays are the KF2 -> KF1 direction.  match12[i1] = i2 for mutually consistent pairs.
  int SearchBySim3(const FrameArrays& KF1, const FrameArrays& KF2, const std::vector<float>& mvScaleFactors1,
                   const std::vector<float>& mvScaleFactors2, const std::vector<uint8_t>& valid1,
                   const std::vector<float>& u1, const std::vector<float>& v1, const std::vector<int32_t>& level1,
                   const std::vector<uint8_t>& desc1, const std::vector<uint8_t>& valid2, const std::vector<float>& u2,
                   const std::vector<float>& v2, const std::vector<int32_t>& level2, const std::vector<uint8_t>& desc2,
                   float th, std::vector<int32_t>& match12) {
    match12.assign(KF1.N(), -1);
    int32_t n = 0;
    check(orbfe_search_by_sim3(device_, &KF1.c, &KF2.c, mvScaleFactors1.data(), mvScaleFactors2.data(),
                               (int)mvScaleFactors1.size(), valid1.data(), u1.data(), v1.data(), level1.data(),
                               desc1.data(), valid2.data(), u2.data(), v2.data(), level2.data(), desc2.data(), th,
                               match12.data(), &n),
          "SearchBySim3");
    return n;
  }

  float mfNNratio;
  bool mbCheckOrientation;

 private:
  int device_;
};

// MapPoint::mObservations resident on the device (orbfe_obsgraph): point slots are the MapPointTable's, kf slot <-> KeyFrame* is
// the caller's map, as are the spanning tree, mvpMapPoints and the map mutex.  Mutations change the host mirror alone; the
// calls that read the table on the device write the changed rows first.
class ObservationGraph {
 public:
  struct Votes { std::vector<int32_t> kfSlot, weight; };  // ascending kf slot
  struct Connections {  // KeyFrame::UpdateConnections: ids are mnIds
    std::vector<int64_t> orderedId, connectId;
    std::vector<int32_t> orderedWeight, connectWeight;
    int64_t parentId = -1;
  };
  struct NormalDepth { std::vector<float> normal, minDist, maxDist; std::vector<uint8_t> valid; };
  ObservationGraph(int pointCapacity, int kfCapacity, int rowWidth = 64, int device = 0) : kfCap_(kfCapacity) {
    check(orbfe_obsgraph_create(device, pointCapacity, kfCapacity, rowWidth, &h_), "ObservationGraph");
  }
  ~ObservationGraph() { orbfe_obsgraph_destroy(h_); }
  ObservationGraph(const ObservationGraph&) = delete;
  ObservationGraph& operator=(const ObservationGraph&) = delete;
  orbfe_obsgraph* handle() const { return h_; }
  void SetKeyFrames(const std::vector<int32_t>& kfSlot, const std::vector<int64_t>& mnId, const std::vector<float>& Ow,
                    const std::vector<uint8_t>& bad) {
    const size_t n = kfSlot.size();
    if (mnId.size() != n || Ow.size() != 3 * n || bad.size() != n) throw std::invalid_argument("ObservationGraph::SetKeyFrames: one entry per kf slot");
    check(orbfe_obsgraph_set_keyframes(h_, (int)n, kfSlot.data(), mnId.data(), Ow.data(), bad.data()), "ObservationGraph::SetKeyFrames");
  }
  void SetPoints(const std::vector<int32_t>& slot, const std::vector<uint8_t>& bad, const std::vector<int32_t>& refKfSlot) {
    if (bad.size() != slot.size() || refKfSlot.size() != slot.size()) throw std::invalid_argument("ObservationGraph::SetPoints: one entry per slot");
    check(orbfe_obsgraph_set_points(h_, (int)slot.size(), slot.data(), bad.data(), refKfSlot.data()), "ObservationGraph::SetPoints");
  }
  // MapPoint::AddObservation per entry
  void AddObservations(const std::vector<int32_t>& slot, const std::vector<int32_t>& kfSlot, const std::vector<uint16_t>& idx,
                       const std::vector<uint8_t>& octave, const std::vector<uint8_t>& stereo) {
    const size_t n = slot.size();
    if (kfSlot.size() != n || idx.size() != n || octave.size() != n || stereo.size() != n)
      throw std::invalid_argument("ObservationGraph::AddObservations: one entry per observation");
    check(orbfe_obsgraph_add_observations(h_, (int)n, slot.data(), kfSlot.data(), idx.data(), octave.data(), stereo.data()),
          "ObservationGraph::AddObservations");
  }
  // MapPoint::EraseObservation per entry; returns became-bad flags
  std::vector<uint8_t> EraseObservations(const std::vector<int32_t>& slot, const std::vector<int32_t>& kfSlot) {
    if (kfSlot.size() != slot.size()) throw std::invalid_argument("ObservationGraph::EraseObservations: one kf slot per slot");
    std::vector<uint8_t> bad(slot.size() + 1, 0);
    check(orbfe_obsgraph_erase_observations(h_, (int)slot.size(), slot.data(), kfSlot.data(), bad.data()), "ObservationGraph::EraseObservations");
    bad.resize(slot.size());
    return bad;
  }
  // the map-point part of KeyFrame::SetBadFlag; returns the slots of the points that became bad
  std::vector<int32_t> EraseKeyFrame(int kfSlot) {
    int n = 0;
    std::vector<int32_t> out;
    int rc = orbfe_obsgraph_erase_keyframe(h_, kfSlot, nullptr, 0, &n);
    if (rc == ORBFE_ERR_CAPACITY) {
      out.resize((size_t)n);
      rc = orbfe_obsgraph_erase_keyframe(h_, kfSlot, out.data(), n, &n);
    }
    check(rc, "ObservationGraph::EraseKeyFrame");
    out.resize((size_t)n);
    return out;
  }
  // the votes of one point-slot list (a key frame's: self = its kf slot; a frame's: self = -1)
  Votes VotesOf(const std::vector<int32_t>& pointSlots, int selfKfSlot = -1) const {
    const int32_t off[2] = {0, (int32_t)pointSlots.size()}, self = selfKfSlot;
    Votes v;
    v.kfSlot.assign((size_t)kfCap_, 0); v.weight.assign((size_t)kfCap_, 0);
    int32_t count = 0;
    check(orbfe_obsgraph_votes(h_, 1, off, pointSlots.data(), &self, kfCap_, v.kfSlot.data(), v.weight.data(), &count), "ObservationGraph::VotesOf");
    v.kfSlot.resize((size_t)count); v.weight.resize((size_t)count);
    return v;
  }
  // KeyFrame::UpdateConnections :347-393 on a key frame's votes; mnIdOfSlot: kf slot -> mnId
  static Connections UpdateConnections(const Votes& v, const std::vector<int64_t>& mnIdOfSlot) {
    const size_t n = v.kfSlot.size();
    std::vector<int64_t> id(n + 1);
    for (size_t i = 0; i < n; i++) id[i] = mnIdOfSlot.at((size_t)v.kfSlot[i]);
    Connections c;
    c.orderedId.assign(n + 1, 0); c.orderedWeight.assign(n + 1, 0); c.connectId.assign(n + 1, 0); c.connectWeight.assign(n + 1, 0);
    int no = 0, nc = 0;
    check(orbfe_obsgraph_update_connections((int)n, id.data(), v.weight.data(), c.orderedId.data(), c.orderedWeight.data(), &no,
                                            c.connectId.data(), c.connectWeight.data(), &nc, &c.parentId), "ObservationGraph::UpdateConnections");
    c.orderedId.resize((size_t)no); c.orderedWeight.resize((size_t)no); c.connectId.resize((size_t)nc); c.connectWeight.resize((size_t)nc);
    return c;
  }
  // LocalMapping::KeyFrameCulling's counts: candidate c = kfSlot[c] with features slot / octave [offsets[c], offsets[c+1])
  void CullingCounts(const std::vector<int32_t>& kfSlot, const std::vector<int32_t>& offsets, const std::vector<int32_t>& slot,
                     const std::vector<uint8_t>& octave, std::vector<int32_t>& nMPs, std::vector<int32_t>& nRedundant) const {
    if (offsets.size() != kfSlot.size() + 1 || slot.size() != octave.size() || (size_t)offsets.back() != slot.size())
      throw std::invalid_argument("ObservationGraph::CullingCounts: the lists disagree in length");
    nMPs.assign(kfSlot.size(), 0); nRedundant.assign(kfSlot.size(), 0);
    check(orbfe_obsgraph_culling_counts(h_, (int)kfSlot.size(), kfSlot.data(), offsets.data(), slot.data(), octave.data(), nMPs.data(),
                                        nRedundant.data()), "ObservationGraph::CullingCounts");
  }
  // MapPoint::UpdateNormalAndDepth at the given positions (3 floats per slot)
  NormalDepth UpdateNormalAndDepth(const std::vector<int32_t>& slot, const std::vector<float>& pos, const std::vector<float>& mvScaleFactors) const {
    const size_t n = slot.size();
    if (pos.size() != 3 * n) throw std::invalid_argument("ObservationGraph::UpdateNormalAndDepth: one position per slot");
    NormalDepth r;
    r.normal.assign(3 * n + 1, 0); r.minDist.assign(n + 1, 0); r.maxDist.assign(n + 1, 0); r.valid.assign(n + 1, 0);
    check(orbfe_obsgraph_update_normal_depth(h_, (int)n, slot.data(), pos.data(), mvScaleFactors.data(), (int)mvScaleFactors.size(),
                                             r.normal.data(), r.minDist.data(), r.maxDist.data(), r.valid.data()), "ObservationGraph::UpdateNormalAndDepth");
    r.normal.resize(3 * n); r.minDist.resize(n); r.maxDist.resize(n); r.valid.resize(n);
    return r;
  }

  // ---- KeyFrame::mvpMapPoints: key frame -> its points (rows of kfRowWidth point slots, -1 = NULL) ----
  void EnableKeyFramePoints(int kfRowWidth) {
    check(orbfe_obsgraph_enable_keyframe_points(h_, kfRowWidth), "ObservationGraph::EnableKeyFramePoints");
    kfRowWidth_ = kfRowWidth;
  }
  // the whole mvpMapPoints of a key frame, as at the KeyFrame constructor
  void SetKeyFramePoints(int kfSlot, const std::vector<int32_t>& slot) {
    check(orbfe_obsgraph_set_keyframe_points(h_, kfSlot, (int)slot.size(), slot.data()), "ObservationGraph::SetKeyFramePoints");
  }
  // KeyFrame::AddMapPoint / ReplaceMapPointMatch (slot) and EraseMapPointMatch(idx) (slot -1) per entry, all or nothing
  void AssignKeyFramePoints(const std::vector<int32_t>& kfSlot, const std::vector<uint16_t>& idx, const std::vector<int32_t>& slot) {
    if (idx.size() != kfSlot.size() || slot.size() != kfSlot.size())
      throw std::invalid_argument("ObservationGraph::AssignKeyFramePoints: one entry per assignment");
    check(orbfe_obsgraph_assign_keyframe_points(h_, (int)kfSlot.size(), kfSlot.data(), idx.data(), slot.data()),
          "ObservationGraph::AssignKeyFramePoints");
  }
  std::vector<int32_t> GetKeyFramePoints(int kfSlot, bool fromDevice = false) const {
    std::vector<int32_t> out((size_t)std::max(kfRowWidth_, 1), -1);
    int32_t n = 0;
    check(orbfe_obsgraph_get_keyframe_points(h_, fromDevice ? 1 : 0, kfSlot, out.data(), &n), "ObservationGraph::GetKeyFramePoints");
    out.resize((size_t)n);
    return out;
  }
  // the ordered union of the key frames' map points per query (query q: kfSlots [offsets[q], offsets[q+1])); a first call
  // sized by `capacity` (<= 0: 4096) is repeated once with the largest count when a list does not fit
  std::vector<std::vector<int32_t>> KeyFramePointsUnion(const std::vector<int32_t>& offsets, const std::vector<int32_t>& kfSlots,
                                                        int capacity = 0) const {
    if (offsets.empty() || (size_t)offsets.back() != kfSlots.size())
      throw std::invalid_argument("ObservationGraph::KeyFramePointsUnion: the lists disagree in length");
    const size_t Q = offsets.size() - 1;
    size_t cap = capacity > 0 ? (size_t)capacity : 4096;
    std::vector<int32_t> out(Q * cap + 1), count(Q + 1, 0);
    int rc = orbfe_obsgraph_keyframe_points_union(h_, (int)Q, offsets.data(), kfSlots.data(), (int)cap, out.data(), count.data());
    if (rc == ORBFE_ERR_CAPACITY) {
      cap = (size_t)*std::max_element(count.begin(), count.end());
      out.assign(Q * cap + 1, 0);
      rc = orbfe_obsgraph_keyframe_points_union(h_, (int)Q, offsets.data(), kfSlots.data(), (int)cap, out.data(), count.data());
    }
    check(rc, "ObservationGraph::KeyFramePointsUnion");
    std::vector<std::vector<int32_t>> lists(Q);
    for (size_t q = 0; q < Q; q++) lists[q].assign(out.begin() + (ptrdiff_t)(q * cap), out.begin() + (ptrdiff_t)(q * cap + (size_t)count[q]));
    return lists;
  }
  // Tracking::UpdateLocalPoints: mvpLocalKeyFrames as kf slots -> mvpLocalMapPoints as point slots, the slot list of
  // MapPointTable::SearchLocalPoints
  std::vector<int32_t> UpdateLocalPoints(const std::vector<int32_t>& localKfSlots, int capacity = 0) const {
    return KeyFramePointsUnion({0, (int32_t)localKfSlots.size()}, localKfSlots, capacity)[0];
  }
  // KeyFrame::TrackedMapPoints(minObs) per kf slot
  std::vector<int32_t> TrackedMapPoints(const std::vector<int32_t>& kfSlot, int minObs) const {
    std::vector<int32_t> count(kfSlot.size() + 1, 0);
    check(orbfe_obsgraph_tracked_points(h_, (int)kfSlot.size(), kfSlot.data(), minObs, count.data()), "ObservationGraph::TrackedMapPoints");
    count.resize(kfSlot.size());
    return count;
  }

  // ---- KeyFrame::mDescriptors per kf slot, and MapPoint::ComputeDistinctiveDescriptors over the rows ----
  void EnableKeyFrameDescriptors(int kfDescWidth) {
    check(orbfe_obsgraph_enable_keyframe_descriptors(h_, kfDescWidth), "ObservationGraph::EnableKeyFrameDescriptors");
    kfDescWidth_ = kfDescWidth;
  }
  // mDescriptors of a key frame, 32 bytes per row, from the host; unlike the other mutations this touches the device
  void SetKeyFrameDescriptors(int kfSlot, const std::vector<uint8_t>& desc) {
    if (desc.size() % 32) throw std::invalid_argument("ObservationGraph::SetKeyFrameDescriptors: 32 bytes per descriptor");
    check(orbfe_obsgraph_set_keyframe_descriptors(h_, kfSlot, (int)(desc.size() / 32), desc.data()), "ObservationGraph::SetKeyFrameDescriptors");
  }
  // ... or from a resident frame (FrameArrays::resident()), device to device; the frame may be released afterwards
  void SetKeyFrameDescriptors(int kfSlot, const orbfe_frame* frame) {
    check(orbfe_obsgraph_set_keyframe_descriptors_frame(h_, kfSlot, frame), "ObservationGraph::SetKeyFrameDescriptors");
  }
  std::vector<uint8_t> GetKeyFrameDescriptors(int kfSlot) const {
    std::vector<uint8_t> out((size_t)std::max(kfDescWidth_, 1) * 32, 0);
    int32_t n = 0;
    check(orbfe_obsgraph_get_keyframe_descriptors(h_, kfSlot, out.data(), &n), "ObservationGraph::GetKeyFrameDescriptors");
    out.resize((size_t)n * 32);
    return out;
  }
  // per slot the winner's (kf slot, idx) and its 32 bytes; -1 / -1 / zeros where valid is 0
  struct Distinctive {
    std::vector<int32_t> kfSlot, idx;
    std::vector<uint8_t> desc, valid;
  };
  Distinctive ComputeDistinctiveDescriptors(const std::vector<int32_t>& slot) const {
    const size_t n = slot.size();
    Distinctive r;
    r.kfSlot.assign(n + 1, -1); r.idx.assign(n + 1, -1); r.desc.assign(32 * n + 1, 0); r.valid.assign(n + 1, 0);
    check(orbfe_obsgraph_distinctive_descriptors(h_, (int)n, slot.data(), r.kfSlot.data(), r.idx.data(), r.desc.data(), r.valid.data()),
          "ObservationGraph::ComputeDistinctiveDescriptors");
    r.kfSlot.resize(n); r.idx.resize(n); r.desc.resize(32 * n); r.valid.resize(n);
    return r;
  }

 private:
  orbfe_obsgraph* h_ = nullptr;
  int kfCap_ = 0, kfRowWidth_ = 0, kfDescWidth_ = 0;
};

// The map points Tracking::SearchLocalPoints reads, resident on the device (orbfe_mappoints): slot <-> MapPoint* is the
// caller's map, as the key-frame ids of the KeyFrameDatabase are.
class MapPointTable {
 public:
  // what Frame::isInFrustum leaves on the MapPoints, as arrays over the slot list
  struct Projection {
    std::vector<uint8_t> mbTrackInView;
    std::vector<int32_t> mnTrackScaleLevel;
    std::vector<float> mTrackViewCos, mTrackProjX, mTrackProjY, mTrackProjXR, invZ, dist;
  };
  explicit MapPointTable(int capacity, int device = 0) { check(orbfe_mappoints_create(device, capacity, &h_), "MapPointTable"); }
  ~MapPointTable() { orbfe_mappoints_destroy(h_); }
  MapPointTable(const MapPointTable&) = delete;
  MapPointTable& operator=(const MapPointTable&) = delete;
  int capacity() const { return orbfe_mappoints_capacity(h_); }
  // pos / normal: 3 floats per slot; desc: 32 bytes per slot, or empty to keep the descriptors; flags: ORBFE_MP_BAD | ORBFE_MP_OBSERVED
  void update(const std::vector<int32_t>& slot, const std::vector<float>& pos, const std::vector<float>& normal,
              const std::vector<float>& minDist, const std::vector<float>& maxDist, const std::vector<uint8_t>& desc,
              const std::vector<uint8_t>& flags) {
    const size_t n = slot.size();
    if (pos.size() != 3 * n || normal.size() != 3 * n || minDist.size() != n || maxDist.size() != n || flags.size() != n ||
        (!desc.empty() && desc.size() != 32 * n))
      throw std::invalid_argument("MapPointTable::update: one entry per slot");
    check(orbfe_mappoints_update(h_, (int)n, slot.data(), pos.data(), normal.data(), minDist.data(), maxDist.data(),
                                 desc.empty() ? nullptr : desc.data(), flags.data()), "MapPointTable::update");
  }
  // Frame::isInFrustum(pMP, viewingCosLimit) for every slot; skip: empty, or one byte per slot
  Projection ProjectInFrustum(const std::vector<int32_t>& slot, const orbfe_camera_pose& pose, float viewingCosLimit = 0.5f,
                              const std::vector<uint8_t>& skip = {}) const {
    const size_t n = slot.size();
    if (!skip.empty() && skip.size() != n) throw std::invalid_argument("MapPointTable::ProjectInFrustum: one skip entry per slot");
    Projection p;
    p.mbTrackInView.assign(n, 0); p.mnTrackScaleLevel.assign(n, 0);
    p.mTrackViewCos.assign(n, 0); p.mTrackProjX.assign(n, 0); p.mTrackProjY.assign(n, 0); p.mTrackProjXR.assign(n, 0);
    p.invZ.assign(n, 0); p.dist.assign(n, 0);
    check(orbfe_project_in_frustum(h_, (int)n, slot.data(), skip.empty() ? nullptr : skip.data(), &pose, viewingCosLimit,
                                   p.mbTrackInView.data(), p.mnTrackScaleLevel.data(), p.mTrackViewCos.data(), p.mTrackProjX.data(),
                                   p.mTrackProjY.data(), p.mTrackProjXR.data(), p.invZ.data(), p.dist.data()), "ProjectInFrustum");
    return p;
  }
  // Tracking::SearchLocalPoints: isInFrustum + SearchByProjection(F, points, th) in one call.  match[idx] = position in `slot`
  // of the point given to keypoint idx, or -1; inView (may be NULL) for IncreaseVisible.  Returns nmatches.
  int SearchLocalPoints(const FrameArrays& F, const std::vector<int32_t>& slot, const orbfe_camera_pose& pose,
                        const std::vector<float>& mvScaleFactors, float th, float nnratio, std::vector<int32_t>& match,
                        std::vector<uint8_t>* inView = nullptr, float viewingCosLimit = 0.5f, const std::vector<uint8_t>& skip = {},
                        const std::vector<uint8_t>& blocked = {}) const {
    const size_t n = slot.size();
    if (!skip.empty() && skip.size() != n) throw std::invalid_argument("MapPointTable::SearchLocalPoints: one skip entry per slot");
    if (!blocked.empty() && blocked.size() != (size_t)F.c.n) throw std::invalid_argument("MapPointTable::SearchLocalPoints: one blocked entry per keypoint");
    match.assign((size_t)F.c.n, -1);
    if (inView) inView->assign(n, 0);
    int32_t nmatches = 0;
    check(orbfe_search_local_points(h_, (int)n, slot.data(), skip.empty() ? nullptr : skip.data(), &pose, viewingCosLimit, &F.c,
                                    mvScaleFactors.data(), (int)mvScaleFactors.size(), blocked.empty() ? nullptr : blocked.data(), th,
                                    nnratio, match.data(), &nmatches, inView ? inView->data() : nullptr), "SearchLocalPoints");
    return nmatches;
  }
  // ORBmatcher::Fuse for slot[] against K key frames in one call (orbfe_fuse_mappoints): bestIdx[k * n + i] = the keypoint of
  // KFs[k] Fuse would take for point i, or -1.  chi2Gate: Fuse(pKF, vpMapPoints, th), needs mvInvLevelSigma2; otherwise the
  // Sim3 overload with the caller's decomposition of Scw in pose[k].  graph (may be NULL) + kfSlot: IsInKeyFrame from the
  // observation rows; skip: empty, or K * n bytes; projected (may be NULL): the points that passed the prologue.  Replace /
  // AddObservation / AddMapPoint stay with the caller; the results are those of the state at entry (include/orbfe.h).
  std::vector<int32_t> Fuse(const std::vector<const FrameArrays*>& KFs, const std::vector<orbfe_camera_pose>& pose,
                            const std::vector<int32_t>& slot, const std::vector<float>& mvScaleFactors,
                            const std::vector<float>& mvInvLevelSigma2, float th = 3.0f, bool chi2Gate = true,
                            const ObservationGraph* graph = nullptr, const std::vector<int32_t>& kfSlot = {},
                            const std::vector<uint8_t>& skip = {}, std::vector<uint8_t>* projected = nullptr) const {
    const size_t n = slot.size(), K = KFs.size();
    if (pose.size() != K) throw std::invalid_argument("MapPointTable::Fuse: one pose per key frame");
    if (graph && kfSlot.size() != K) throw std::invalid_argument("MapPointTable::Fuse: one kf slot per key frame");
    if (!skip.empty() && skip.size() != K * n) throw std::invalid_argument("MapPointTable::Fuse: K * n skip entries");
    if (chi2Gate && mvInvLevelSigma2.size() != mvScaleFactors.size())
      throw std::invalid_argument("MapPointTable::Fuse: one mvInvLevelSigma2 entry per level");
    std::vector<const orbfe_frame_view*> views;
    for (const FrameArrays* f : KFs) views.push_back(&f->c);
    std::vector<int32_t> best(K * n + 1, -1);
    if (projected) projected->assign(K * n + 1, 0);
    check(orbfe_fuse_mappoints(h_, graph ? graph->handle() : nullptr, (int)n, slot.data(), (int)K, views.data(),
                               graph ? kfSlot.data() : nullptr, pose.data(), skip.empty() ? nullptr : skip.data(), mvScaleFactors.data(),
                               chi2Gate ? mvInvLevelSigma2.data() : nullptr, (int)mvScaleFactors.size(), th, chi2Gate ? 1 : 0, best.data(),
                               projected ? projected->data() : nullptr), "MapPointTable::Fuse");
    best.resize(K * n);
    if (projected) projected->resize(K * n);
    return best;
  }
  // the prologue of SearchByProjection(CurrentFrame, LastFrame, th, bMono) for the compact list slot[] / lastOctave[]
  // (orbfe_project_last_frame); the fields are 0 where valid is
  struct LastFrameProjection {
    std::vector<uint8_t> valid;
    std::vector<float> u, v, invZ, ur, radius;
  };
  LastFrameProjection ProjectLastFrame(const std::vector<int32_t>& slot, const std::vector<int32_t>& lastOctave,
                                       const orbfe_camera_pose& pose, const std::vector<float>& mvScaleFactors, float th, int mode = 0,
                                       const std::vector<uint8_t>& skip = {}) const {
    const size_t n = slot.size();
    if (lastOctave.size() != n || (!skip.empty() && skip.size() != n))
      throw std::invalid_argument("MapPointTable::ProjectLastFrame: one octave (and skip entry) per slot");
    LastFrameProjection p;
    p.valid.assign(n + 1, 0);
    for (std::vector<float>* a : {&p.u, &p.v, &p.invZ, &p.ur, &p.radius}) a->assign(n + 1, 0.0f);
    check(orbfe_project_last_frame(h_, (int)n, slot.data(), skip.empty() ? nullptr : skip.data(), lastOctave.data(), &pose,
                                   mvScaleFactors.data(), (int)mvScaleFactors.size(), th, mode, p.valid.data(), p.u.data(), p.v.data(),
                                   p.invZ.data(), p.ur.data(), p.radius.data()), "MapPointTable::ProjectLastFrame");
    p.valid.resize(n);
    for (std::vector<float>* a : {&p.u, &p.v, &p.invZ, &p.ur, &p.radius}) a->resize(n);
    return p;
  }
  // SearchByProjection(CurrentFrame, LastFrame, th, bMono) in one call (orbfe_search_last_frame_mappoints): slot[] names the
  // last frame's features with a non-outlier map point in ascending order, lastOctave / lastAngle their mvKeysUn; mode from
  // tlc (0 / 1 bForward / 2 bBackward).  match[i2] = position in slot[] of the point given to keypoint i2 of Cur, or -1 -- the
  // `match` of PoseOptimization below.  Returns nmatches; the 2 * th retry and the bookkeeping behind stay with the caller.
  int SearchByProjectionLastFrame(const FrameArrays& Cur, const std::vector<int32_t>& slot, const std::vector<int32_t>& lastOctave,
                                  const std::vector<float>& lastAngle, const orbfe_camera_pose& pose,
                                  const std::vector<float>& mvScaleFactors, float th, int mode, std::vector<int32_t>& match,
                                  bool checkOrientation = true, const std::vector<uint8_t>& skip = {},
                                  const std::vector<uint8_t>& blocked = {}, std::vector<uint8_t>* valid = nullptr) const {
    const size_t n = slot.size();
    if (lastOctave.size() != n || (checkOrientation && lastAngle.size() != n) || (!skip.empty() && skip.size() != n))
      throw std::invalid_argument("MapPointTable::SearchByProjectionLastFrame: one octave, angle (and skip entry) per slot");
    if (!blocked.empty() && blocked.size() != (size_t)Cur.c.n)
      throw std::invalid_argument("MapPointTable::SearchByProjectionLastFrame: one blocked entry per keypoint");
    match.assign((size_t)Cur.c.n + 1, -1);
    if (valid) valid->assign(n + 1, 0);
    int32_t nmatches = 0;
    check(orbfe_search_last_frame_mappoints(h_, (int)n, slot.data(), skip.empty() ? nullptr : skip.data(), lastOctave.data(),
                                            checkOrientation ? lastAngle.data() : nullptr, &pose, &Cur.c, mvScaleFactors.data(),
                                            (int)mvScaleFactors.size(), blocked.empty() ? nullptr : blocked.data(), mode, th,
                                            checkOrientation ? 1 : 0, match.data(), &nmatches, valid ? valid->data() : nullptr),
          "MapPointTable::SearchByProjectionLastFrame");
    match.resize((size_t)Cur.c.n);
    if (valid) valid->resize(n);
    return nmatches;
  }
  // the prologue of SearchByProjection(CurrentFrame, pKF_k, sAlreadyFound, th, ORBdist) for K candidates in one launch
  // (orbfe_project_keyframe): candidate k owns entries [offsets[k], offsets[k + 1]) of slot / skip and pose[k]
  struct KeyFrameProjection {
    std::vector<uint8_t> valid;
    std::vector<float> u, v, invZ, dist;
    std::vector<int32_t> level;
  };
  KeyFrameProjection ProjectKeyFrames(const std::vector<int32_t>& offsets, const std::vector<int32_t>& slot,
                                      const std::vector<orbfe_camera_pose>& pose, const std::vector<uint8_t>& skip = {}) const {
    const size_t K = pose.size(), n = slot.size();
    if (offsets.size() != K + 1 || (size_t)offsets.back() != n || (!skip.empty() && skip.size() != n))
      throw std::invalid_argument("MapPointTable::ProjectKeyFrames: K + 1 offsets that end at the number of slots");
    KeyFrameProjection p;
    p.valid.assign(n + 1, 0); p.level.assign(n + 1, 0);
    for (std::vector<float>* a : {&p.u, &p.v, &p.invZ, &p.dist}) a->assign(n + 1, 0.0f);
    check(orbfe_project_keyframe(h_, (int)K, offsets.data(), slot.data(), skip.empty() ? nullptr : skip.data(), pose.data(),
                                 p.valid.data(), p.u.data(), p.v.data(), p.invZ.data(), p.level.data(), p.dist.data()),
          "MapPointTable::ProjectKeyFrames");
    p.valid.resize(n); p.level.resize(n);
    for (std::vector<float>* a : {&p.u, &p.v, &p.invZ, &p.dist}) a->resize(n);
    return p;
  }
  // Tracking::Relocalization's SearchByProjection for K candidates in one call (orbfe_search_keyframe_mappoints_multi):
  // match[k * Cur.n + i2] = position in candidate k's part of slot[] or -1; nMatches[k].  kfAngle: pKF_k->mvKeysUn[.].angle
  // over the concatenated list; blocked: empty, or K * Cur.n bytes (Cur.mvpMapPoints[i2] != NULL at the entry of call k).
  std::vector<int32_t> SearchByProjectionKeyFrames(const FrameArrays& Cur, const std::vector<int32_t>& offsets,
                                                   const std::vector<int32_t>& slot, const std::vector<float>& kfAngle,
                                                   const std::vector<orbfe_camera_pose>& pose, const std::vector<float>& mvScaleFactors,
                                                   const std::vector<float>& th, const std::vector<int32_t>& ORBdist,
                                                   std::vector<int32_t>& match, bool checkOrientation = true,
                                                   const std::vector<uint8_t>& skip = {}, const std::vector<uint8_t>& blocked = {}) const {
    const size_t K = pose.size(), n = slot.size(), nc = (size_t)Cur.c.n;
    if (offsets.size() != K + 1 || (size_t)offsets.back() != n || th.size() != K || ORBdist.size() != K ||
        (checkOrientation && kfAngle.size() != n) || (!skip.empty() && skip.size() != n) || (!blocked.empty() && blocked.size() != K * nc))
      throw std::invalid_argument("MapPointTable::SearchByProjectionKeyFrames: the lists disagree in length");
    std::vector<const uint8_t*> blk;
    for (size_t k = 0; k < K && !blocked.empty(); k++) blk.push_back(blocked.data() + k * nc);
    match.assign(K * nc + 1, -1);
    std::vector<int32_t> nMatches(K + 1, 0);
    check(orbfe_search_keyframe_mappoints_multi(h_, &Cur.c, mvScaleFactors.data(), (int)mvScaleFactors.size(), (int)K, offsets.data(),
                                                slot.data(), skip.empty() ? nullptr : skip.data(),
                                                checkOrientation ? kfAngle.data() : nullptr, pose.data(), blk.empty() ? nullptr : blk.data(),
                                                th.data(), ORBdist.data(), checkOrientation ? 1 : 0, match.data(), nMatches.data()),
          "MapPointTable::SearchByProjectionKeyFrames");
    match.resize(K * nc);
    nMatches.resize(K);
    return nMatches;
  }
  // ORBmatcher::SearchBySim3 for K candidates of KF1 in one call (orbfe_search_by_sim3_mappoints_multi): slot1 = KF1's
  // GetMapPointMatches() in slot space (-1 = none, one entry per keypoint), candidate k owns [offsets2[k], offsets2[k + 1]) of
  // slot2 (one entry per keypoint of KF2s[k]); legs12[k] / legs21[k] are the two directions, composed by the caller
  // (include/orbfe.h: orbfe_sim3_leg).  matched12In: empty, or K * N1 slots of vpMatches12_k at entry (-1 = NULL).
  // vbAlreadyMatched2: already2 (empty, or one byte per entry of slot2) and / or, with graph and kf2Slot, GetIndexInKeyFrame from
  // the observation rows.  match12[k * N1 + i1] = i2 or -1; returns nFound per candidate.
  std::vector<int32_t> SearchBySim3(const FrameArrays& KF1, const std::vector<int32_t>& slot1, const std::vector<const FrameArrays*>& KF2s,
                                    const std::vector<int32_t>& offsets2, const std::vector<int32_t>& slot2,
                                    const std::vector<orbfe_sim3_leg>& legs12, const std::vector<orbfe_sim3_leg>& legs21,
                                    const std::vector<float>& mvScaleFactors1, const std::vector<float>& mvScaleFactors2, float th,
                                    std::vector<int32_t>& match12, const std::vector<int32_t>& matched12In = {},
                                    const ObservationGraph* graph = nullptr, const std::vector<int32_t>& kf2Slot = {},
                                    const std::vector<uint8_t>& already2 = {}) const {
    const size_t K = KF2s.size(), n1 = slot1.size();
    if (offsets2.size() != K + 1 || (size_t)offsets2.back() != slot2.size() || legs12.size() != K || legs21.size() != K ||
        n1 != (size_t)KF1.c.n || (!matched12In.empty() && matched12In.size() != K * n1) || (graph && kf2Slot.size() != K) ||
        (!already2.empty() && already2.size() != slot2.size()) || mvScaleFactors1.size() != mvScaleFactors2.size())
      throw std::invalid_argument("MapPointTable::SearchBySim3: the lists disagree in length");
    std::vector<const orbfe_frame_view*> views;
    for (const FrameArrays* f : KF2s) views.push_back(&f->c);
    match12.assign(K * n1 + 1, -1);
    std::vector<int32_t> nFound(K + 1, 0);
    check(orbfe_search_by_sim3_mappoints_multi(h_, graph ? graph->handle() : nullptr, &KF1.c, slot1.data(), (int)K, views.data(),
                                               offsets2.data(), slot2.data(), legs12.data(), legs21.data(),
                                               matched12In.empty() ? nullptr : matched12In.data(), graph ? kf2Slot.data() : nullptr,
                                               already2.empty() ? nullptr : already2.data(), mvScaleFactors1.data(), mvScaleFactors2.data(),
                                               (int)mvScaleFactors1.size(), th, match12.data(), nFound.data()),
          "MapPointTable::SearchBySim3");
    match12.resize(K * n1);
    nFound.resize(K);
    return nFound;
  }
  // SearchByProjection(pKF, Scw, vpPoints, vpMatched, th) in one call (orbfe_search_by_projection_sim3_mappoints): slot[] =
  // vpPoints in slot space, pose = the caller's decomposition of Scw (as for Fuse's Sim3 overload); matched: empty, or one byte
  // per keypoint (vpMatched[idx] != NULL); skip: empty, or one byte per slot (spAlreadyFound).  match[idx] = position in slot[] of
  // the point newly given to keypoint idx, or -1.  Returns nmatches.
  int SearchByProjection(const FrameArrays& KF, const orbfe_camera_pose& pose, const std::vector<int32_t>& slot,
                         const std::vector<float>& mvScaleFactors, float th, std::vector<int32_t>& match,
                         const std::vector<uint8_t>& matched = {}, const std::vector<uint8_t>& skip = {},
                         std::vector<uint8_t>* projected = nullptr) const {
    const size_t n = slot.size();
    if ((!skip.empty() && skip.size() != n) || (!matched.empty() && matched.size() != (size_t)KF.c.n))
      throw std::invalid_argument("MapPointTable::SearchByProjection: one skip entry per slot, one matched entry per keypoint");
    match.assign((size_t)KF.c.n + 1, -1);
    if (projected) projected->assign(n + 1, 0);
    int32_t nmatches = 0;
    check(orbfe_search_by_projection_sim3_mappoints(h_, (int)n, slot.data(), skip.empty() ? nullptr : skip.data(), &pose, &KF.c,
                                                    mvScaleFactors.data(), (int)mvScaleFactors.size(),
                                                    matched.empty() ? nullptr : matched.data(), th, match.data(), &nmatches,
                                                    projected ? projected->data() : nullptr),
          "MapPointTable::SearchByProjection");
    match.resize((size_t)KF.c.n);
    if (projected) projected->resize(n);
    return nmatches;
  }
  orbfe_mappoints* handle() const { return h_; }
  // the tail of Optimizer::OptimizeEssentialGraph (:1070-1103) on the table: the position of slot[p] becomes
  // Sout[r]^-1 .map(Scw[r] .map(P)), r = refVertex[p] (-1: left alone); Scw / SiwOut 8 doubles per vertex
  void EssentialGraphCorrect(const std::vector<int32_t>& slot, const std::vector<double>& Scw, const std::vector<double>& SiwOut,
                             const std::vector<int32_t>& refVertex) {
    if (Scw.size() != SiwOut.size() || Scw.size() % 8 || slot.size() != refVertex.size())
      throw std::invalid_argument("MapPointTable::EssentialGraphCorrect: the lists disagree in length");
    check(orbfe_essential_graph_correct_mappoints(h_, (int)(Scw.size() / 8), Scw.data(), SiwOut.data(), (int)slot.size(), slot.data(),
                                                  refVertex.data()), "MapPointTable::EssentialGraphCorrect");
  }
  // GetWorldPos of slot[] as the table holds it (3 floats each)
  std::vector<float> Positions(const std::vector<int32_t>& slot) const {
    std::vector<float> out(3 * slot.size() + 1);
    check(orbfe_mappoints_positions(h_, (int)slot.size(), slot.data(), out.data()), "MapPointTable::Positions");
    out.resize(3 * slot.size());
    return out;
  }

  // MapPoint::UpdateNormalAndDepth for slot[] on the device: positions from this table, normal / min / max into it; returns valid[]
  std::vector<uint8_t> UpdateNormalAndDepth(const ObservationGraph& graph, const std::vector<int32_t>& slot, const std::vector<float>& mvScaleFactors) {
    std::vector<uint8_t> valid(slot.size() + 1, 0);
    check(orbfe_obsgraph_update_normal_depth_mappoints(graph.handle(), h_, (int)slot.size(), slot.data(), mvScaleFactors.data(),
                                                       (int)mvScaleFactors.size(), valid.data()), "MapPointTable::UpdateNormalAndDepth");
    valid.resize(slot.size());
    return valid;
  }
  // MapPoint::ComputeDistinctiveDescriptors for slot[] on the device: the rows and the key frames' descriptors from `graph`,
  // the winners' bytes into this table's descriptors; returns valid[] (winners: the winning (kf slot, idx) per slot, -1 where
  // valid is 0)
  std::vector<uint8_t> ComputeDistinctiveDescriptors(const ObservationGraph& graph, const std::vector<int32_t>& slot,
                                                     std::vector<int32_t>* winnerKfSlot = nullptr, std::vector<int32_t>* winnerIdx = nullptr) {
    std::vector<uint8_t> valid(slot.size() + 1, 0);
    if (winnerKfSlot) winnerKfSlot->assign(slot.size() + 1, -1);
    if (winnerIdx) winnerIdx->assign(slot.size() + 1, -1);
    check(orbfe_obsgraph_distinctive_descriptors_mappoints(graph.handle(), h_, (int)slot.size(), slot.data(),
                                                           winnerKfSlot ? winnerKfSlot->data() : nullptr, winnerIdx ? winnerIdx->data() : nullptr,
                                                           valid.data()), "MapPointTable::ComputeDistinctiveDescriptors");
    valid.resize(slot.size());
    if (winnerKfSlot) winnerKfSlot->resize(slot.size());
    if (winnerIdx) winnerIdx->resize(slot.size());
    return valid;
  }
  // The point loop at the head of LoopClosing::CorrectLoop (src/LoopClosing.cc:558-600) with UpdateNormalAndDepth, on the
  // table (orbfe_correct_loop_mappoints): kfSlot = the key frames in visiting order (ascending mnId recommended), corrected /
  // noncorrected 8 doubles each (LoopClosing::CorrectedSim3s), OwCorrected 3 floats each, skip = the slots with
  // mnCorrectedByKF == current.  slots: the claimed slots in claim order; ref: the claimant's place in the list; valid:
  // normal and range were rewritten.  The graph's Ow of the listed key frames are OwCorrected afterwards.
  struct LoopCorrection {
    std::vector<int32_t> slots, ref;
    std::vector<uint8_t> valid;
  };
  LoopCorrection CorrectLoop(const ObservationGraph& graph, const std::vector<int32_t>& kfSlot, const std::vector<double>& corrected,
                             const std::vector<double>& noncorrected, const std::vector<float>& OwCorrected,
                             const std::vector<float>& mvScaleFactors, const std::vector<int32_t>& skip = {}) {
    const size_t K = kfSlot.size();
    if (corrected.size() != 8 * K || noncorrected.size() != 8 * K || OwCorrected.size() != 3 * K)
      throw std::invalid_argument("MapPointTable::CorrectLoop: one entry per key frame");
    LoopCorrection out;
    size_t cap = 1024;
    for (;;) {  // a count above the capacity changes nothing: grow to it and repeat
      out.slots.assign(cap, 0); out.ref.assign(cap, 0); out.valid.assign(cap, 0);
      int32_t n = 0;
      const int rc = orbfe_correct_loop_mappoints(graph.handle(), h_, (int)K, kfSlot.data(), corrected.data(), noncorrected.data(),
                                                  OwCorrected.data(), (int)skip.size(), skip.data(), mvScaleFactors.data(),
                                                  (int)mvScaleFactors.size(), (int)cap, out.slots.data(), out.ref.data(),
                                                  out.valid.data(), &n);
      if (rc == ORBFE_ERR_CAPACITY && (size_t)n > cap) { cap = (size_t)n; continue; }
      check(rc, "MapPointTable::CorrectLoop");
      out.slots.resize((size_t)n); out.ref.resize((size_t)n); out.valid.resize((size_t)n);
      return out;
    }
  }
  // The map-point loop at the tail of LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:818-852) on the table
  // (orbfe_gba_update_mappoints): slot = GetAllMapPoints (distinct), inGBA / posGBA (3 floats) aligned with it; kfSlot a compact
  // list with reached, TcwBef = mTcwBefGBA and TwcNew = GetPoseInverse() after SetPose (16 floats each).  Returns moved[]: 0
  // skipped, 1 took posGBA, 2 moved through its reference key frame.
  std::vector<uint8_t> GlobalBundleAdjustmentUpdate(const ObservationGraph& graph, const std::vector<int32_t>& slot,
                                                    const std::vector<uint8_t>& inGBA, const std::vector<float>& posGBA,
                                                    const std::vector<int32_t>& kfSlot, const std::vector<uint8_t>& reached,
                                                    const std::vector<float>& TcwBef, const std::vector<float>& TwcNew) {
    const size_t n = slot.size(), m = kfSlot.size();
    if (inGBA.size() != n || posGBA.size() != 3 * n || reached.size() != m || TcwBef.size() != 16 * m || TwcNew.size() != 16 * m)
      throw std::invalid_argument("MapPointTable::GlobalBundleAdjustmentUpdate: the lists disagree in length");
    std::vector<uint8_t> moved(n + 1, 0);
    check(orbfe_gba_update_mappoints(graph.handle(), h_, (int)n, slot.data(), inGBA.data(), posGBA.data(), (int)m, kfSlot.data(),
                                     reached.data(), TcwBef.data(), TwcNew.data(), moved.data()),
          "MapPointTable::GlobalBundleAdjustmentUpdate");
    moved.resize(n);
    return moved;
  }
  // Where stereo / RGB-D map points are born, on the table (orbfe_create_stereo_points): Tracking::StereoInitialization
  // (src/Tracking.cc:563-578, mode ORBFE_STEREO_ALL), the depth-sorted loop of Tracking::CreateNewKeyFrame (:1182-1234,
  // ORBFE_STEREO_KEYFRAME) and of Tracking::UpdateLastFrame (:899-949, ORBFE_STEREO_TEMPORAL; graph may be NULL).  F must
  // be resident; mvDepth one entry per keypoint; newSlot = free slots, taken in creation order (its size is the capacity);
  // occupied (mvpMapPoints[i] && Observations() >= 1) and stale (a point with Observations() < 1) may be empty.  In modes
  // ALL and KEYFRAME the graph receives the points, their observation by kfSlot and -- with key-frame rows enabled --
  // kfSlot's mvpMapPoints entries.  More created points than newSlot holds throws with neither table touched.
  struct StereoPoints {
    std::vector<int32_t> idx, slot;  // keypoint index and slot of each created point, in creation order
    std::vector<uint8_t> cleared;    // KEYFRAME: mvpMapPoints[i] was dropped before the new point took its place
    int walked = 0;                  // candidates handled before the stop
  };
  StereoPoints CreateStereoPoints(const ObservationGraph* graph, const FrameArrays& F, int kfSlot, const orbfe_camera_pose& pose,
                                  const std::vector<float>& mvDepth, float mThDepth, int mode, const std::vector<float>& mvScaleFactors,
                                  const std::vector<int32_t>& newSlot, const std::vector<uint8_t>& occupied = {},
                                  const std::vector<uint8_t>& stale = {}) {
    const size_t n = mvDepth.size();
    if ((!occupied.empty() && occupied.size() != n) || (!stale.empty() && stale.size() != n))
      throw std::invalid_argument("MapPointTable::CreateStereoPoints: one mask entry per keypoint");
    StereoPoints out;
    out.idx.assign(newSlot.size() + 1, 0); out.slot.assign(newSlot.size() + 1, 0); out.cleared.assign(n + 1, 0);
    int32_t created = 0, walked = 0;
    check(orbfe_create_stereo_points(h_, graph ? graph->handle() : nullptr, F.resident(), kfSlot, &pose, (int)n, mvDepth.data(),
                                     occupied.empty() ? nullptr : occupied.data(), stale.empty() ? nullptr : stale.data(), mThDepth,
                                     mode, mvScaleFactors.data(), (int)mvScaleFactors.size(), newSlot.data(), (int)newSlot.size(),
                                     out.idx.data(), out.slot.data(), out.cleared.data(), &created, &walked),
          "MapPointTable::CreateStereoPoints");
    out.idx.resize((size_t)created); out.slot.resize((size_t)created); out.cleared.resize(n);
    out.walked = walked;
    return out;
  }
  // LocalMapping::CreateNewMapPoints' pair loop and the birth at its tail (src/LocalMapping.cc:331-501) on the table, in one
  // call (orbfe_create_triangulated_points).  KF1 / neighbours must be resident; kf1Slot / kf2Slot are their kf slots in
  // `graph`; match12 [k * n1 + i1] as SearchForTriangulationMulti returns it; newSlot = free slots, taken in creation order
  // (its size is the capacity).  The graph receives the points, both observations and -- with key-frame rows enabled -- both
  // key frames' mvpMapPoints entries.  More created points than newSlot holds throws with neither table touched.
  struct CreatedTriangulatedPoints {
    std::vector<int32_t> k, i1, i2, slot;  // the pair and the slot of each created point, in creation order
    std::vector<uint8_t> status;           // [k * n1 + i1], ORBFE_TRI_*
    std::vector<int32_t> perNeighbour;     // points made with neighbour k
  };
  CreatedTriangulatedPoints CreateTriangulatedPoints(const ObservationGraph& graph, const FrameArrays& KF1, int kf1Slot,
                                                     const KeyFrameCamera& cam1, const std::vector<const FrameArrays*>& neighbours,
                                                     const std::vector<int32_t>& kf2Slot, const std::vector<const KeyFrameCamera*>& cams,
                                                     const std::vector<int32_t>& match12, const std::vector<float>& mvScaleFactors,
                                                     const std::vector<float>& mvLevelSigma2, float ratioFactor,
                                                     const std::vector<int32_t>& newSlot) {
    const size_t K = neighbours.size(), n1 = (size_t)KF1.N(), cap = newSlot.size();
    if (kf2Slot.size() != K || cams.size() != K || match12.size() != K * n1 || mvLevelSigma2.size() != mvScaleFactors.size())
      throw std::invalid_argument("MapPointTable::CreateTriangulatedPoints: one kf slot, camera and match row per neighbour");
    std::vector<const orbfe_frame*> frames(K + 1, nullptr);
    std::vector<orbfe_keyframe_camera> cc(K + 1);
    for (size_t k = 0; k < K; k++) { frames[k] = neighbours[k]->resident(); cc[k] = cams[k]->c(); }
    const orbfe_keyframe_camera c1 = cam1.c();
    CreatedTriangulatedPoints out;
    out.k.assign(cap + 1, 0); out.i1.assign(cap + 1, 0); out.i2.assign(cap + 1, 0); out.slot.assign(cap + 1, 0);
    out.status.assign(K * n1 + 1, 0); out.perNeighbour.assign(K + 1, 0);
    int32_t created = 0;
    check(orbfe_create_triangulated_points(h_, graph.handle(), KF1.resident(), kf1Slot, &c1, (int)K, frames.data(), kf2Slot.data(), cc.data(),
                                           match12.data(), mvScaleFactors.data(), mvLevelSigma2.data(), (int)mvScaleFactors.size(),
                                           ratioFactor, newSlot.data(), (int)cap, out.k.data(), out.i1.data(), out.i2.data(),
                                           out.slot.data(), out.status.data(), out.perNeighbour.data(), &created),
          "MapPointTable::CreateTriangulatedPoints");
    const size_t m = (size_t)created;
    out.k.resize(m); out.i1.resize(m); out.i2.resize(m); out.slot.resize(m); out.status.resize(K * n1); out.perNeighbour.resize(K);
    return out;
  }
  // GetDescriptor of slot[] as the table holds it (32 bytes each)
  std::vector<uint8_t> Descriptors(const std::vector<int32_t>& slot) const {
    std::vector<uint8_t> out(32 * slot.size() + 1);
    check(orbfe_mappoints_descriptors(h_, (int)slot.size(), slot.data(), out.data()), "MapPointTable::Descriptors");
    out.resize(32 * slot.size());
    return out;
  }

 private:
  orbfe_mappoints* h_ = nullptr;
};

// The host parts of LoopClosing::CorrectLoop (src/LoopClosing.cc:519-551, :590-596) and of the key-frame walk at the tail of
// LoopClosing::RunGlobalBundleAdjustment (:788-815); the resident parts are MapPointTable::CorrectLoop and
// MapPointTable::GlobalBundleAdjustmentUpdate.  Poses are row-major 4 x 4 floats, Sim3 records qx qy qz qw tx ty tz s.
class LoopClosing {
 public:
  struct Sim3s {
    std::vector<double> corrected, noncorrected;  // CorrectedSim3 / NonCorrectedSim3, 8 doubles per key frame
    std::vector<float> TiwCorrected;              // what SetPose receives (:600), 16 floats per key frame
  };
  // Tiw = GetPose() of mvpCurrentConnectedKFs, TwcCur = mpCurrentKF->GetPoseInverse(), cur = its index, Scw = mg2oScw
  static Sim3s CorrectedSim3s(const std::vector<float>& Tiw, const std::vector<float>& TwcCur, int cur, const std::vector<double>& Scw) {
    if (Tiw.size() % 16 || TwcCur.size() != 16 || Scw.size() != 8)
      throw std::invalid_argument("LoopClosing::CorrectedSim3s: 16 floats per pose, 8 doubles for Scw");
    const size_t K = Tiw.size() / 16;
    Sim3s out;
    out.corrected.assign(8 * K + 1, 0.0); out.noncorrected.assign(8 * K + 1, 0.0); out.TiwCorrected.assign(16 * K + 1, 0.f);
    check(orbfe_correct_loop_sim3s((int)K, Tiw.data(), TwcCur.data(), cur, Scw.data(), out.corrected.data(), out.noncorrected.data(),
                                   out.TiwCorrected.data()), "LoopClosing::CorrectedSim3s");
    out.corrected.resize(8 * K); out.noncorrected.resize(8 * K); out.TiwCorrected.resize(16 * K);
    return out;
  }
  struct Propagation {
    std::vector<float> TcwNew;              // mTcwGBA after the walk, 16 floats per key frame
    std::vector<uint8_t> reached, visited;  // mnBAGlobalForKF == nLoopKF after the walk; the key frame receives SetPose
  };
  // origins = mvpKeyFrameOrigins as indices; the children of key frame k = child[childOffsets[k] .. childOffsets[k + 1]);
  // Tcw / Twc at entry, inGBA[k] = mnBAGlobalForKF == nLoopKF at entry, TcwGBA = mTcwGBA
  static Propagation PropagateGBA(const std::vector<int32_t>& origins, const std::vector<int32_t>& childOffsets,
                                  const std::vector<int32_t>& child, const std::vector<float>& Tcw, const std::vector<float>& Twc,
                                  const std::vector<uint8_t>& inGBA, const std::vector<float>& TcwGBA) {
    const size_t n = inGBA.size();
    if (Tcw.size() != 16 * n || Twc.size() != 16 * n || TcwGBA.size() != 16 * n || childOffsets.size() != n + 1 ||
        (size_t)std::max(childOffsets.back(), 0) > child.size())
      throw std::invalid_argument("LoopClosing::PropagateGBA: the lists disagree in length");
    Propagation out;
    out.TcwNew.assign(16 * n + 1, 0.f); out.reached.assign(n + 1, 0); out.visited.assign(n + 1, 0);
    check(orbfe_gba_propagate_keyframes((int)n, (int)origins.size(), origins.data(), childOffsets.data(), child.data(), Tcw.data(),
                                        Twc.data(), inGBA.data(), TcwGBA.data(), out.TcwNew.data(), out.reached.data(),
                                        out.visited.data()), "LoopClosing::PropagateGBA");
    out.TcwNew.resize(16 * n); out.reached.resize(n); out.visited.resize(n);
    return out;
  }
};

// The host definitions behind MapPointTable::CreateStereoPoints and the close-point counts of Tracking::NeedNewKeyFrame
// (src/Tracking.cc:1100-1114); neither needs a device.
class Tracking {
 public:
  struct StereoSelection {
    std::vector<int32_t> idx;                  // created keypoints, in creation order
    std::vector<float> pos, normal;            // 3 floats each
    std::vector<float> minDist, maxDist;       // the raw mfMinDistance / mfMaxDistance
    std::vector<uint8_t> cleared;
    int walked = 0;
  };
  // orbfe_stereo_points_select: x / y / octave = mvKeysUn, centre = the camera centre normal and range are taken from (the
  // key frame's; pose.Ow for the temporal points); occupied / stale may be empty
  static StereoSelection SelectStereoPoints(const std::vector<float>& x, const std::vector<float>& y, const std::vector<int32_t>& octave,
                                            const std::vector<float>& mvDepth, const orbfe_camera_pose& pose, float mThDepth, int mode,
                                            const std::vector<float>& mvScaleFactors, const float centre[3],
                                            const std::vector<uint8_t>& occupied = {}, const std::vector<uint8_t>& stale = {}) {
    const size_t n = mvDepth.size();
    if (x.size() != n || y.size() != n || octave.size() != n || (!occupied.empty() && occupied.size() != n) ||
        (!stale.empty() && stale.size() != n))
      throw std::invalid_argument("Tracking::SelectStereoPoints: one entry per keypoint");
    StereoSelection out;
    out.idx.assign(n + 1, 0); out.pos.assign(3 * n + 1, 0.f); out.normal.assign(3 * n + 1, 0.f);
    out.minDist.assign(n + 1, 0.f); out.maxDist.assign(n + 1, 0.f); out.cleared.assign(n + 1, 0);
    int32_t created = 0, walked = 0;
    check(orbfe_stereo_points_select((int)n, x.data(), y.data(), octave.data(), mvDepth.data(), occupied.empty() ? nullptr : occupied.data(),
                                     stale.empty() ? nullptr : stale.data(), &pose, mThDepth, mode, mvScaleFactors.data(),
                                     (int)mvScaleFactors.size(), centre, (int)n, out.idx.data(), out.pos.data(), out.normal.data(),
                                     out.minDist.data(), out.maxDist.data(), out.cleared.data(), &created, &walked),
          "Tracking::SelectStereoPoints");
    const size_t m = (size_t)created;
    out.idx.resize(m); out.pos.resize(3 * m); out.normal.resize(3 * m); out.minDist.resize(m); out.maxDist.resize(m);
    out.cleared.resize(n);
    out.walked = walked;
    return out;
  }
  // (nTrackedClose, nNonTrackedClose): 0 < mvDepth[i] < mThDepth; hasPoint[i] = mvpMapPoints[i] != NULL, outlier = mvbOutlier
  static std::pair<int, int> CountClosePoints(const std::vector<float>& mvDepth, const std::vector<uint8_t>& hasPoint,
                                              const std::vector<uint8_t>& outlier, float mThDepth) {
    if (hasPoint.size() != mvDepth.size() || outlier.size() != mvDepth.size())
      throw std::invalid_argument("Tracking::CountClosePoints: one entry per keypoint");
    int32_t tracked = 0, nonTracked = 0;
    check(orbfe_count_close_points((int)mvDepth.size(), mvDepth.data(), hasPoint.data(), outlier.data(), mThDepth, &tracked, &nonTracked),
          "Tracking::CountClosePoints");
    return {tracked, nonTracked};
  }
};

// Optimizer::PoseOptimization (src/Optimizer.cc:256-473), Optimizer::OptimizeSim3 (:1116-1323), Optimizer::LocalBundleAdjustment
// (:483-814), Optimizer::BundleAdjustment (:54-253) and Optimizer::OptimizeEssentialGraph (:833-1104) on the device.
// Both forms return nInitialCorrespondences - nBad, write the pose Frame::SetPose receives into Tcw (row-major 4 x 4) and
// mvbOutlier of every edge; with fewer than 3 edges they return 0 and leave both alone.
class Optimizer {
 public:
  // one edge per entry: Xw 3 floats each, (u, v) = mvKeysUn[i].pt, uRight = mvuRight[i] (< 0: monocular), invSigma2 =
  // mvInvLevelSigma2[octave]; K5 = fx fy cx cy mbf
  static int PoseOptimization(const std::vector<float>& Xw, const std::vector<float>& u, const std::vector<float>& v,
                              const std::vector<float>& uRight, const std::vector<float>& invSigma2, const float K5[5], float Tcw[16],
                              std::vector<uint8_t>& mvbOutlier, orbfe_poseopt_stats* stats = nullptr, int device = 0) {
    const size_t n = u.size();
    if (Xw.size() != 3 * n || v.size() != n || uRight.size() != n || invSigma2.size() != n)
      throw std::invalid_argument("Optimizer::PoseOptimization: one entry per edge");
    mvbOutlier.resize(n, 0);
    float out[16];
    int32_t nInliers = 0;
    check(orbfe_pose_optimization(device, (int)n, Xw.data(), u.data(), v.data(), uRight.data(), invSigma2.data(), K5, Tcw, out,
                                  mvbOutlier.data(), &nInliers, stats, nullptr), "PoseOptimization");
    for (int k = 0; k < 16; k++) Tcw[k] = out[k];
    return nInliers;
  }
  // on the resident table, with the match[] MapPointTable::SearchLocalPoints returned for F and slot: keypoints without an
  // edge (no match, or a bad slot) keep their mvbOutlier entry
  static int PoseOptimization(const MapPointTable& table, const std::vector<int32_t>& slot, const FrameArrays& F,
                              const std::vector<int32_t>& match, const std::vector<float>& mvInvLevelSigma2, const float K5[5],
                              float Tcw[16], std::vector<uint8_t>& mvbOutlier, orbfe_poseopt_stats* stats = nullptr) {
    if (match.size() != (size_t)F.c.n) throw std::invalid_argument("Optimizer::PoseOptimization: one match entry per keypoint");
    mvbOutlier.resize((size_t)F.c.n, 0);
    float out[16];
    int32_t nInliers = 0;
    check(orbfe_pose_optimization_mappoints(table.handle(), (int)slot.size(), slot.data(), &F.c, match.data(), mvInvLevelSigma2.data(),
                                            (int)mvInvLevelSigma2.size(), K5, Tcw, out, mvbOutlier.data(), &nInliers, stats, nullptr),
          "PoseOptimization");
    for (int k = 0; k < 16; k++) Tcw[k] = out[k];
    return nInliers;
  }

  // OptimizeSim3 without the map graph.  The caller walks vpMatches1 as the reference does (:1173-1259) and hands in, for the
  // pairs it adds edges for: idx1 (vnIndexEdge: the index i into vpMatches1), X1 / X2 3 floats each (P3D1c = R1w * P3D1w +
  // t1w, P3D2c likewise), obs1 / obs2 2 floats each (mvKeysUn[i].pt of key frame 1, mvKeysUn[i2].pt of key frame 2), the
  // two mvInvLevelSigma2[octave], K1 / K2 = fx fy cx cy.  vpMatches1 holds whatever the caller keeps per keypoint of key
  // frame 1 (here an index, -1 = no match): every erased pair gets vpMatches1[idx1[i]] = -1, also when the call returns 0
  // early.  S12 = g2o::Sim3's members qx qy qz qw tx ty tz s, in and out; it is left untouched when the reference would
  // leave g2oS12 untouched (fewer than 10 pairs left after round one, or no pair).  Returns nIn.
  static int OptimizeSim3(const std::vector<int32_t>& idx1, const std::vector<float>& X1, const std::vector<float>& X2,
                          const std::vector<float>& obs1, const std::vector<float>& obs2, const std::vector<float>& invSigma2_1,
                          const std::vector<float>& invSigma2_2, const float K1[4], const float K2[4], std::vector<int32_t>& vpMatches1,
                          double S12[8], float th2, bool bFixScale, orbfe_optsim3_stats* stats = nullptr, int device = 0) {
    const size_t n = idx1.size();
    if (X1.size() != 3 * n || X2.size() != 3 * n || obs1.size() != 2 * n || obs2.size() != 2 * n || invSigma2_1.size() != n ||
        invSigma2_2.size() != n)
      throw std::invalid_argument("Optimizer::OptimizeSim3: one entry per pair");
    for (int32_t i : idx1)
      if (i < 0 || (size_t)i >= vpMatches1.size()) throw std::invalid_argument("Optimizer::OptimizeSim3: idx1 outside vpMatches1");
    float rec[13];
    sim3_record(S12, rec);
    std::vector<uint8_t> bad(n ? n : 1, 0);
    double out[8];
    int32_t nIn = 0;
    orbfe_optsim3_stats st;
    check(orbfe_optimize_sim3(device, (int)n, X1.data(), X2.data(), obs1.data(), obs2.data(), invSigma2_1.data(), invSigma2_2.data(),
                              K1, K2, rec, th2, bFixScale ? 1 : 0, out, bad.data(), &nIn, &st, nullptr, nullptr), "OptimizeSim3");
    for (size_t i = 0; i < n; i++)
      if (bad[i]) vpMatches1[(size_t)idx1[i]] = -1;
    if (st.rounds == 2)
      for (int k = 0; k < 8; k++) S12[k] = out[k];
    if (stats) *stats = st;
    return nIn;
  }
  // What the map-graph walk of LocalBundleAdjustment (:485-536) or BundleAdjustment (:62-140) found, flattened: the nLocal
  // local key frames first, then the fixed ones (Tcw row-major 4 x 4 floats, cam = fx fy cx cy mbf each); localIsFixed[j] =
  // (mnId == 0), empty = none; the points; one edge per observation, grouped by point in the order the reference adds them
  // (u, v = mvKeysUn[idx].pt, uRight = mvuRight[idx] (< 0: monocular), invSigma2 = mvInvLevelSigma2[octave])
  struct BundleGraph {
    int nLocal = 0;
    std::vector<float> Tcw, cam;
    std::vector<uint8_t> localIsFixed;
    std::vector<float> Xw;
    std::vector<int32_t> edgePose, edgePoint;
    std::vector<float> u, v, uRight, invSigma2;
    void validate(const char* who) const {
      const size_t nT = Tcw.size() / 16, nE = edgePose.size();
      if (nLocal < 0 || Tcw.size() != 16 * nT || (size_t)nLocal > nT || cam.size() != 5 * nT || Xw.size() % 3 != 0 ||
          (!localIsFixed.empty() && localIsFixed.size() != (size_t)nLocal))
        throw std::invalid_argument(std::string(who) + ": one Tcw and cam per key frame, one localIsFixed per local one");
      if (edgePoint.size() != nE || u.size() != nE || v.size() != nE || uRight.size() != nE || invSigma2.size() != nE)
        throw std::invalid_argument(std::string(who) + ": one entry per edge");
    }
  };
  // LocalBundleAdjustment from :538 on.  Returns per edge whether the reference puts the pair into vToErase (the caller runs
  // EraseMapPointMatch / EraseObservation under its map mutex); TcwOut [nLocal * 16] is what SetPose receives, XwOut
  // [nPoints * 3] what SetWorldPos receives, both in double.  stats->stopped && stats->rounds == 0: the early return of :689
  static std::vector<uint8_t> LocalBundleAdjustment(const BundleGraph& g, std::vector<double>& TcwOut, std::vector<double>& XwOut,
                                                    const volatile int* pbStopFlag = nullptr, orbfe_lba_stats* stats = nullptr,
                                                    int device = 0) {
    g.validate("Optimizer::LocalBundleAdjustment");
    const size_t nE = g.edgePose.size();
    TcwOut.assign(16 * (size_t)g.nLocal + 1, 0.0);
    XwOut.assign(g.Xw.size() + 1, 0.0);
    std::vector<uint8_t> erase(nE ? nE : 1, 0);
    check(orbfe_local_bundle_adjustment(device, g.nLocal, (int)(g.Tcw.size() / 16) - g.nLocal, g.Tcw.data(),
                                        g.localIsFixed.empty() ? nullptr : g.localIsFixed.data(), g.cam.data(), (int)(g.Xw.size() / 3),
                                        g.Xw.data(), (int)nE, g.edgePose.data(), g.edgePoint.data(), g.u.data(), g.v.data(),
                                        g.uRight.data(), g.invSigma2.data(), pbStopFlag, TcwOut.data(), XwOut.data(), erase.data(),
                                        nullptr, stats, nullptr), "LocalBundleAdjustment");
    TcwOut.resize(16 * (size_t)g.nLocal); XwOut.resize(g.Xw.size()); erase.resize(nE);
    return erase;
  }
  // BundleAdjustment: one optimize(nIterations), Huber kernels with bRobust, no classification
  static void BundleAdjustment(const BundleGraph& g, std::vector<double>& TcwOut, std::vector<double>& XwOut, int nIterations = 5,
                               const volatile int* pbStopFlag = nullptr, bool bRobust = true, orbfe_lba_stats* stats = nullptr,
                               int device = 0) {
    g.validate("Optimizer::BundleAdjustment");
    TcwOut.assign(16 * (size_t)g.nLocal + 1, 0.0);
    XwOut.assign(g.Xw.size() + 1, 0.0);
    check(orbfe_bundle_adjustment(device, g.nLocal, (int)(g.Tcw.size() / 16) - g.nLocal, g.Tcw.data(),
                                  g.localIsFixed.empty() ? nullptr : g.localIsFixed.data(), g.cam.data(), (int)(g.Xw.size() / 3), g.Xw.data(),
                                  (int)g.edgePose.size(), g.edgePose.data(), g.edgePoint.data(), g.u.data(), g.v.data(), g.uRight.data(),
                                  g.invSigma2.data(), nIterations, bRobust ? 1 : 0, pbStopFlag, TcwOut.data(), XwOut.data(), stats, nullptr),
          "BundleAdjustment");
    TcwOut.resize(16 * (size_t)g.nLocal); XwOut.resize(g.Xw.size());
  }
  // OptimizeEssentialGraph (:833-1104) from the graph on.  The caller flattens its key frames into vertices (vScw: the
  // CorrectedSim3 entry or Sim3(Rcw, tcw, 1); Snc: the NonCorrectedSim3 entry or vScw; qx qy qz qw tx ty tz s) and its four
  // edge loops into (edgeI, edgeJ, edgeKind): kind 1 for the new LoopConnections (:907-936, measured from vScw), kind 0 for
  // spanning tree, old loops and covisibility (:939-1040, measured from Snc).  The de-duplication rules stay the caller's.
  struct EssentialGraph {
    std::vector<double> Scw, Snc;  // 8 per vertex; Snc empty: the same as Scw
    std::vector<uint8_t> isFixed;  // per vertex (pKF == pLoopKF); empty: none
    std::vector<int32_t> edgeI, edgeJ;
    std::vector<uint8_t> edgeKind;  // per edge; empty: all 0
    void validate(const char* what) const {
      const size_t n = Scw.size() / 8;
      if (Scw.empty() || Scw.size() % 8 || (!Snc.empty() && Snc.size() != Scw.size()) || (!isFixed.empty() && isFixed.size() != n) ||
          edgeJ.size() != edgeI.size() || (!edgeKind.empty() && edgeKind.size() != edgeI.size()))
        throw std::invalid_argument(std::string(what) + ": the flattened lists disagree in length");
    }
  };
  // -> CorrectedSiw per vertex in SiwOut (8 doubles each) and the pose SetPose receives in TiwOut (row-major 4 x 4 floats)
  static void OptimizeEssentialGraph(const EssentialGraph& g, std::vector<double>& SiwOut, std::vector<float>& TiwOut, bool bFixScale,
                                     int nIterations = 20, orbfe_essgraph_stats* stats = nullptr, int device = 0) {
    g.validate("Optimizer::OptimizeEssentialGraph");
    const size_t n = g.Scw.size() / 8;
    SiwOut.assign(8 * n, 0.0);
    TiwOut.assign(16 * n, 0.0f);
    check(orbfe_optimize_essential_graph(device, (int)n, g.Scw.data(), g.Snc.empty() ? nullptr : g.Snc.data(),
                                         g.isFixed.empty() ? nullptr : g.isFixed.data(), (int)g.edgeI.size(), g.edgeI.data(), g.edgeJ.data(),
                                         g.edgeKind.empty() ? nullptr : g.edgeKind.data(), bFixScale ? 1 : 0, nIterations, SiwOut.data(),
                                         TiwOut.data(), nullptr, stats),
          "OptimizeEssentialGraph");
  }
  // the point correction of its tail (:1070-1103) on arrays: refVertex[p] = the vertex of the point's reference key frame, -1 bad
  static std::vector<float> EssentialGraphCorrectPoints(const EssentialGraph& g, const std::vector<double>& SiwOut, const std::vector<float>& Xw,
                                                        const std::vector<int32_t>& refVertex, int device = 0) {
    if (SiwOut.size() != g.Scw.size() || Xw.size() != 3 * refVertex.size())
      throw std::invalid_argument("Optimizer::EssentialGraphCorrectPoints: the lists disagree in length");
    std::vector<float> out(Xw.size() + 1);
    check(orbfe_essential_graph_correct_points(device, (int)(g.Scw.size() / 8), g.Scw.data(), SiwOut.data(), (int)refVertex.size(), Xw.data(),
                                               refVertex.data(), out.data()), "EssentialGraphCorrectPoints");
    out.resize(Xw.size());
    return out;
  }
  // K candidates in one launch: pairOff [K + 1], K1 / K2 4 K floats, S12 8 K doubles, th2 and bFixScale one entry each; idx1
  // indexes the candidate's own vpMatches1[k].  Returns nIn of every candidate
  static std::vector<int> OptimizeSim3Multi(const std::vector<int32_t>& pairOff, const std::vector<int32_t>& idx1,
                                            const std::vector<float>& X1, const std::vector<float>& X2, const std::vector<float>& obs1,
                                            const std::vector<float>& obs2, const std::vector<float>& invSigma2_1,
                                            const std::vector<float>& invSigma2_2, const std::vector<float>& K1,
                                            const std::vector<float>& K2, std::vector<std::vector<int32_t>>& vpMatches1,
                                            std::vector<double>& S12, const std::vector<float>& th2,
                                            const std::vector<uint8_t>& bFixScale, std::vector<orbfe_optsim3_stats>* stats = nullptr,
                                            int device = 0) {
    if (pairOff.empty() || pairOff[0] != 0) throw std::invalid_argument("Optimizer::OptimizeSim3Multi: pairOff holds K + 1 entries from 0");
    const size_t K = pairOff.size() - 1, n = idx1.size();
    if ((size_t)pairOff[K] != n || X1.size() != 3 * n || X2.size() != 3 * n || obs1.size() != 2 * n || obs2.size() != 2 * n ||
        invSigma2_1.size() != n || invSigma2_2.size() != n)
      throw std::invalid_argument("Optimizer::OptimizeSim3Multi: one entry per pair");
    if (K1.size() != 4 * K || K2.size() != 4 * K || S12.size() != 8 * K || th2.size() != K || bFixScale.size() != K ||
        vpMatches1.size() != K)
      throw std::invalid_argument("Optimizer::OptimizeSim3Multi: one entry per candidate");
    for (size_t k = 0; k < K; k++) {
      if (pairOff[k + 1] < pairOff[k]) throw std::invalid_argument("Optimizer::OptimizeSim3Multi: pairOff must not descend");
      for (int32_t p = pairOff[k]; p < pairOff[k + 1]; p++)
        if (idx1[(size_t)p] < 0 || (size_t)idx1[(size_t)p] >= vpMatches1[k].size())
          throw std::invalid_argument("Optimizer::OptimizeSim3Multi: idx1 outside vpMatches1");
    }
    std::vector<float> rec(13 * K + 1);
    for (size_t k = 0; k < K; k++) sim3_record(S12.data() + 8 * k, rec.data() + 13 * k);
    std::vector<uint8_t> bad(n ? n : 1, 0);
    std::vector<double> out(8 * K + 1);
    std::vector<int32_t> nIn(K + 1, 0);
    std::vector<orbfe_optsim3_stats> st(K + 1);
    check(orbfe_optimize_sim3_multi(device, (int)K, pairOff.data(), X1.data(), X2.data(), obs1.data(), obs2.data(), invSigma2_1.data(),
                                    invSigma2_2.data(), K1.data(), K2.data(), rec.data(), th2.data(), bFixScale.data(), out.data(),
                                    bad.data(), nIn.data(), st.data(), nullptr, nullptr), "OptimizeSim3Multi");
    std::vector<int> ret(K);
    for (size_t k = 0; k < K; k++) {
      for (int32_t p = pairOff[k]; p < pairOff[k + 1]; p++)
        if (bad[(size_t)p]) vpMatches1[k][(size_t)idx1[(size_t)p]] = -1;
      if (st[k].rounds == 2)
        for (int j = 0; j < 8; j++) S12[8 * k + j] = out[8 * k + j];
      ret[k] = nIn[k];
    }
    if (stats) stats->assign(st.begin(), st.begin() + (std::ptrdiff_t)K);
    return ret;
  }
  // g2o::Sim3's members -> the sim3[13] record the C-ABI takes (R = r.toRotationMatrix() row-major, t, s; rounded to float
  // as the reference's cv::Mat hand-over is): the C-ABI rebuilds Sim3(Matrix3d, Vector3d, double) from it
  static void sim3_record(const double S[8], float rec[13]) {
    const double x = S[0], y = S[1], z = S[2], w = S[3];
    const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x;
    const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
    const double R[9] = {1.0 - (tyy + tzz), txy - twz, txz + twy, txy + twz, 1.0 - (txx + tzz), tyz - twx,
                         txz - twy, tyz + twx, 1.0 - (txx + tyy)};
    for (int k = 0; k < 9; k++) rec[k] = (float)R[k];
    rec[9] = (float)S[4]; rec[10] = (float)S[5]; rec[11] = (float)S[6]; rec[12] = (float)S[7];
  }
};

// Sim3Solver (src/Sim3Solver.cc) without the map graph: the caller walks vpMatched12 as the reference's constructor does
// (:62-103) and hands in, for the n pairs it keeps, mvnIndices1 (:92), mvX3Dc1 / mvX3Dc2 (3 floats per pair, :95-98), the
// sigma2 of the two keypoints' levels (:84-85), fx fy cx cy of mK1 / mK2, N1 = vpMatched12.size() and bFixScale.  The class
// computes maxErr = (float)(9.210 * sigma2) (:87-88) and calls SetRansacParameters() with the reference's defaults (:111).
// Sim3Solver::evaluate_all evaluates every solver's mRansacMaxIts hypotheses in ONE orbfe_sim3_ransac_multi call; iterate()
// then behaves as the reference's (:150-220) over the results (Sim3Replay, orbfe_sim3_replay.hpp).  The caller's round-robin
// loop (src/LoopClosing.cc:342-404) stays as it is.
class Sim3Solver {
 public:
  Sim3Solver(const std::vector<int32_t>& indices1, const std::vector<float>& x3dc1, const std::vector<float>& x3dc2,
             const std::vector<float>& sigma2_1, const std::vector<float>& sigma2_2, const float cam1[4], const float cam2[4],
             int N1, bool bFixScale)
      : indices1_(indices1), x1_(x3dc1), x2_(x3dc2), fixScale_(bFixScale) {
    const size_t n = indices1.size();
    if (x3dc1.size() != 3 * n || x3dc2.size() != 3 * n || sigma2_1.size() != n || sigma2_2.size() != n)
      throw std::invalid_argument("Sim3Solver: one entry per pair in every array");
    for (int32_t i : indices1)
      if (i < 0 || i >= N1) throw std::invalid_argument("Sim3Solver: indices1 outside [0, N1)");
    e1_.resize(n); e2_.resize(n);
    for (size_t i = 0; i < n; i++) { e1_[i] = (float)(9.210 * sigma2_1[i]); e2_[i] = (float)(9.210 * sigma2_2[i]); }  // :87-88
    std::memcpy(cam1_, cam1, sizeof cam1_); std::memcpy(cam2_, cam2, sizeof cam2_);
    st_.N = (int)n; st_.mN1 = N1;
    SetRansacParameters();
  }
  // :118-142; what an earlier evaluate_all left is dropped (the number of hypotheses may have changed)
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    st_.mRansacMinInliers = minInliers;
    st_.mRansacMaxIts = orbfe_sim3_max_iterations(st_.N, probability, minInliers, maxIterations);
    st_.mnIterations = 0;
    evaluated_ = false;
  }
  int N() const { return st_.N; }
  int maxIterations() const { return st_.mRansacMaxIts; }
  // what evaluate_all evaluates for this solver: nothing when iterate() would return at :156
  int nHypotheses() const { return st_.N < st_.mRansacMinInliers ? 0 : st_.mRansacMaxIts; }

  // triples[k]: 3 * nHypotheses() pair indices of solver k (e.g. orbfe_sim3_triples_from_draws of the reference's stream)
  static void evaluate_all(const std::vector<Sim3Solver*>& solvers, const std::vector<std::vector<int32_t>>& triples, int device = 0) {
    const int K = (int)solvers.size();
    if ((int)triples.size() != K) throw std::invalid_argument("Sim3Solver::evaluate_all: one array of triples per solver");
    std::vector<int32_t> pairOff(1, 0), hypOff(1, 0), tr, wordOff((size_t)K + 1, 0);
    std::vector<float> x1, x2, e1, e2, c1, c2;
    size_t W = 0;
    for (int k = 0; k < K; k++) {
      const Sim3Solver& s = *solvers[k];
      if (s.fixScale_ != solvers[0]->fixScale_) throw std::invalid_argument("Sim3Solver::evaluate_all: the solvers of one call share bFixScale");
      if (triples[k].size() != 3 * (size_t)s.nHypotheses()) throw std::invalid_argument("Sim3Solver::evaluate_all: 3 * nHypotheses() indices per solver");
      pairOff.push_back(pairOff.back() + s.st_.N);
      hypOff.push_back(hypOff.back() + s.nHypotheses());
      x1.insert(x1.end(), s.x1_.begin(), s.x1_.end()); x2.insert(x2.end(), s.x2_.begin(), s.x2_.end());
      e1.insert(e1.end(), s.e1_.begin(), s.e1_.end()); e2.insert(e2.end(), s.e2_.begin(), s.e2_.end());
      c1.insert(c1.end(), s.cam1_, s.cam1_ + 4); c2.insert(c2.end(), s.cam2_, s.cam2_ + 4);
      tr.insert(tr.end(), triples[k].begin(), triples[k].end());
      W += (size_t)s.nHypotheses() * (size_t)((s.st_.N + 31) / 32);
    }
    const int H = hypOff.back();
    std::vector<int32_t> nInl((size_t)H + 1);
    std::vector<uint8_t> status((size_t)H + 1);
    std::vector<float> sim3((size_t)H * 13 + 1);
    std::vector<uint32_t> words(W + 1);
    x1.push_back(0.0f); x2.push_back(0.0f); e1.push_back(0.0f); e2.push_back(0.0f); c1.push_back(0.0f); c2.push_back(0.0f); tr.push_back(0);
    check(orbfe_sim3_ransac_multi(device, K, pairOff.back(), H, pairOff.data(), x1.data(), x2.data(), e1.data(), e2.data(), c1.data(),
                                  c2.data(), K > 0 && solvers[0]->fixScale_ ? 1 : 0, hypOff.data(), tr.data(), nInl.data(),
                                  status.data(), sim3.data(), words.data(), wordOff.data()),
          "Sim3Solver::evaluate_all");
    for (int k = 0; k < K; k++) {
      Sim3Solver& s = *solvers[k];
      const size_t h0 = (size_t)hypOff[k], h1 = (size_t)hypOff[k + 1];
      s.nInliers_.assign(nInl.begin() + h0, nInl.begin() + h1);
      s.status_.assign(status.begin() + h0, status.begin() + h1);
      s.sim3_.assign(sim3.begin() + 13 * h0, sim3.begin() + 13 * h1);
      s.words_.assign(words.begin() + wordOff[k], words.begin() + wordOff[k + 1]);
      s.evaluated_ = true;
    }
  }
  // the triples drawn by the documented generator sim3_seeded_draw through orbfe_sim3_triples_from_draws
  static void evaluate_all(const std::vector<Sim3Solver*>& solvers, uint64_t seed, int device = 0) {
    std::vector<std::vector<int32_t>> triples(solvers.size());
    uint64_t c = 0;
    for (size_t k = 0; k < solvers.size(); k++) {
      const int H = solvers[k]->nHypotheses(), n = solvers[k]->st_.N;
      std::vector<int32_t> draws(3 * (size_t)H);
      for (size_t j = 0; j < draws.size(); j++, c++) draws[j] = sim3_seeded_draw(seed, c, n - (int)(j % 3));
      triples[k].resize(draws.size());
      if (H) check(orbfe_sim3_triples_from_draws(n, H, draws.data(), triples[k].data()), "Sim3Solver::evaluate_all");
    }
    evaluate_all(solvers, triples, device);
  }

  // :150-220 -> true and T12 (row-major 4 x 4) when a hypothesis with more than minInliers inliers came up
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float T12[16]) {
    if (!evaluated_) throw std::logic_error("Sim3Solver::iterate: call Sim3Solver::evaluate_all first");
    const Sim3Replay::Step r = st_.iterate(nIterations, nInliers_.data(), words_.data(), indices1_.data(), vbInliers);
    bNoMore = r.bNoMore;
    nInliers = r.nInliers;
    if (r.best >= 0) {  // :197-202: a copy, so that the estimate outlives the next SetRansacParameters / evaluate_all
      std::memcpy(best_, &sim3_[13 * (size_t)r.best], sizeof best_);
      hasBest_ = true;
    }
    if (r.accepted < 0) return false;
    const float* v = &sim3_[13 * (size_t)r.accepted];
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) T12[4 * i + j] = v[12] * v[3 * i + j];  // :356
      T12[4 * i + 3] = v[9 + i];
    }
    T12[12] = T12[13] = T12[14] = 0.0f; T12[15] = 1.0f;
    return true;
  }
  bool find(std::vector<bool>& vbInliers12, int& nInliers, float T12[16]) {  // :222-226
    bool bFlag;
    return iterate(st_.mRansacMaxIts, bFlag, vbInliers12, nInliers, T12);
  }
  // of the best hypothesis so far (:401-414), which SetRansacParameters and evaluate_all leave alone as the reference leaves
  // mBestRotation; std::logic_error before any hypothesis was taken (the reference returns empty matrices there)
  void GetEstimatedRotation(float R[9]) const { std::memcpy(R, best(), 9 * sizeof(float)); }
  void GetEstimatedTranslation(float t[3]) const { std::memcpy(t, best() + 9, 3 * sizeof(float)); }
  float GetEstimatedScale() const { return best()[12]; }
  int iterations() const { return st_.mnIterations; }
  int bestInliers() const { return st_.mnBestInliers; }

 private:
  std::vector<int32_t> indices1_;
  std::vector<float> x1_, x2_, e1_, e2_;
  float cam1_[4], cam2_[4];
  bool fixScale_;
  Sim3Replay st_;
  bool evaluated_ = false;
  std::vector<int32_t> nInliers_;
  std::vector<uint8_t> status_;
  std::vector<float> sim3_;
  std::vector<uint32_t> words_;
  float best_[13] = {};
  bool hasBest_ = false;
  const float* best() const {
    if (!hasBest_) throw std::logic_error("Sim3Solver: no hypothesis has been taken yet");
    return best_;
  }
};

// PnPsolver (src/PnPsolver.cc) without the map graph: the caller walks vpMapPointMatches as the reference's constructor does
// (:79-101) and hands in, for the n correspondences it keeps, mvP3Dw (3 floats each), mvP2D (mvKeysUn[i].pt, 2 floats each),
// mvSigma2 (mvLevelSigma2 of the key point's octave), mvKeyPointIndices, fx fy cx cy and
// nKeyPoints = vpMapPointMatches.size().  The constructor calls SetRansacParameters() with the reference's defaults (:109).
// PnPsolver::solve_all runs every hypothesis and every Refine() of ALL solvers in ONE orbfe_pnp_solve_multi call (two
// launches); the multi-candidate constructor does that on construction.  iterate() then behaves as the reference's
// (:178-271) over the results (PnPReplay, orbfe_pnp_replay.hpp), so the loop of src/Tracking.cc:1503-1560 stays as it is.
// sets[k]: 4 * nHypotheses() indices, the 4-sets of solver k's hypotheses in order (orbfe_pnp_sets_from_draws of the
// reference's RandomInt stream gives the reference's).  iterate() throws std::out_of_range when it needs more.
class PnPsolver {
 public:
  PnPsolver(const std::vector<float>& p3d, const std::vector<float>& p2d, const std::vector<float>& sigma2,
            const std::vector<int32_t>& keyPointIndices, const float cam[4], int nKeyPoints)
      : p3d_(p3d), p2d_(p2d), sigma2_(sigma2), kp_(keyPointIndices) {
    const size_t n = sigma2.size();
    if (p3d.size() != 3 * n || p2d.size() != 2 * n || keyPointIndices.size() != n)
      throw std::invalid_argument("PnPsolver: one entry per correspondence in every array");
    for (int32_t i : keyPointIndices)
      if (i < 0 || i >= nKeyPoints) throw std::invalid_argument("PnPsolver: keyPointIndices outside [0, nKeyPoints)");
    std::memcpy(cam_, cam, sizeof cam_);
    st_.N = (int)n; st_.nKeyPoints = nKeyPoints;
    SetRansacParameters();
  }
  // :127-164; what an earlier solve_all left is dropped
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                           float epsilon = 0.4f, float th2 = 5.991f) {
    if (minSet != 4) throw std::invalid_argument("PnPsolver: the minimal set is 4");
    st_.SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon);
    st_.mnIterations = 0;
    maxErr_.resize(sigma2_.size());
    for (size_t i = 0; i < sigma2_.size(); i++) maxErr_[i] = sigma2_[i] * th2;  // :163
    solved_ = false;
  }
  int N() const { return st_.N; }
  int minInliers() const { return st_.mRansacMinInliers; }
  int maxIterations() const { return st_.mRansacMaxIts; }
  int iterations() const { return st_.mnIterations; }
  // true: iterate() returns at :186 and the solver takes no part in solve_all
  bool tooFew() const { return st_.N < st_.mRansacMinInliers; }

  static void solve_all(const std::vector<PnPsolver*>& solvers, const std::vector<std::vector<int32_t>>& sets, int device = 0) {
    const int K = (int)solvers.size();
    if ((int)sets.size() != K) throw std::invalid_argument("PnPsolver::solve_all: one array of sets per solver");
    std::vector<int32_t> pointOff(1, 0), hypOff(1, 0), all, minInl, live;
    std::vector<float> p3, p2, me, cam;
    size_t W = 0;
    for (int k = 0; k < K; k++) {
      PnPsolver& s = *solvers[k];
      if (sets[k].size() % 4) throw std::invalid_argument("PnPsolver::solve_all: four indices per hypothesis");
      s.nHyp_ = 0; s.nRec_ = 0; s.solved_ = true;
      if (s.tooFew()) continue;
      live.push_back(k);
      const int H = (int)(sets[k].size() / 4);
      pointOff.push_back(pointOff.back() + s.st_.N);
      hypOff.push_back(hypOff.back() + H);
      p3.insert(p3.end(), s.p3d_.begin(), s.p3d_.end()); p2.insert(p2.end(), s.p2d_.begin(), s.p2d_.end());
      me.insert(me.end(), s.maxErr_.begin(), s.maxErr_.end());
      cam.insert(cam.end(), s.cam_, s.cam_ + 4);
      minInl.push_back(s.st_.mRansacMinInliers);
      all.insert(all.end(), sets[k].begin(), sets[k].end());
      W += (size_t)H * (size_t)((s.st_.N + 31) / 32);
    }
    const int L = (int)live.size(), H = hypOff.back();
    std::vector<int32_t> nInl((size_t)H + 1), wordOff((size_t)L + 1, 0), recOff((size_t)L + 1, 0), recHyp((size_t)H + 1),
        recInl((size_t)H + 1), recWordOff((size_t)L + 1, 0);
    std::vector<uint8_t> status((size_t)H + 1), recStatus((size_t)H + 1);
    std::vector<float> pose((size_t)H * 12 + 1), recPose((size_t)H * 12 + 1);
    std::vector<uint32_t> words(W + 1), recWords(W + 1);
    p3.push_back(0.0f); p2.push_back(0.0f); me.push_back(0.0f); cam.push_back(0.0f); all.push_back(0); minInl.push_back(4);
    check(orbfe_pnp_solve_multi(device, L, pointOff.back(), H, pointOff.data(), p3.data(), p2.data(), me.data(), cam.data(),
                                hypOff.data(), all.data(), minInl.data(), nInl.data(), status.data(), pose.data(), wordOff.data(),
                                words.data(), recOff.data(), recHyp.data(), recInl.data(), recStatus.data(), recPose.data(),
                                recWordOff.data(), recWords.data()),
          "PnPsolver::solve_all");
    for (int j = 0; j < L; j++) {
      PnPsolver& s = *solvers[(size_t)live[j]];
      const size_t h0 = (size_t)hypOff[j], h1 = (size_t)hypOff[j + 1], r0 = (size_t)recOff[j], r1 = (size_t)recOff[j + 1];
      s.nHyp_ = (int)(h1 - h0); s.nRec_ = (int)(r1 - r0);
      s.nInliers_.assign(nInl.begin() + h0, nInl.begin() + h1);
      s.pose_.assign(pose.begin() + 12 * h0, pose.begin() + 12 * h1);
      s.words_.assign(words.begin() + wordOff[j], words.begin() + wordOff[j + 1]);
      s.recHyp_.assign(recHyp.begin() + r0, recHyp.begin() + r1);
      for (int32_t& h : s.recHyp_) h -= (int32_t)h0;  // local to the solver
      s.recInliers_.assign(recInl.begin() + r0, recInl.begin() + r1);
      s.recPose_.assign(recPose.begin() + 12 * r0, recPose.begin() + 12 * r1);
      s.recWords_.assign(recWords.begin() + recWordOff[j], recWords.begin() + recWordOff[j + 1]);
      s.nInliers_.push_back(0); s.words_.push_back(0); s.recHyp_.push_back(0); s.recInliers_.push_back(0); s.recWords_.push_back(0);
    }
  }
  // the multi-candidate form: K solvers built from flattened arrays (candidate k owns correspondences
  // [pointOff[k], pointOff[k + 1]), cam[4 k ..], nKeyPoints[k], sets[k]), parameterised alike and solved in one call
  static std::vector<PnPsolver> make_all(const std::vector<int32_t>& pointOff, const std::vector<float>& p3d,
                                         const std::vector<float>& p2d, const std::vector<float>& sigma2,
                                         const std::vector<int32_t>& keyPointIndices, const std::vector<float>& cam,
                                         const std::vector<int32_t>& nKeyPoints, const std::vector<std::vector<int32_t>>& sets,
                                         double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4,
                                         float epsilon = 0.4f, float th2 = 5.991f, int device = 0) {
    if (pointOff.empty() || pointOff[0] != 0) throw std::invalid_argument("PnPsolver::make_all: pointOff holds K + 1 entries from 0");
    const size_t K = pointOff.size() - 1;
    if (cam.size() != 4 * K || nKeyPoints.size() != K || sets.size() != K || (size_t)pointOff[K] != sigma2.size() ||
        p3d.size() != 3 * sigma2.size() || p2d.size() != 2 * sigma2.size() || keyPointIndices.size() != sigma2.size())
      throw std::invalid_argument("PnPsolver::make_all: the arrays disagree in length");
    std::vector<PnPsolver> out;
    out.reserve(K);
    for (size_t k = 0; k < K; k++) {
      if (pointOff[k + 1] < pointOff[k]) throw std::invalid_argument("PnPsolver::make_all: pointOff must not descend");
      const size_t a = (size_t)pointOff[k], b = (size_t)pointOff[k + 1];
      out.emplace_back(std::vector<float>(p3d.begin() + 3 * a, p3d.begin() + 3 * b), std::vector<float>(p2d.begin() + 2 * a, p2d.begin() + 2 * b),
                       std::vector<float>(sigma2.begin() + a, sigma2.begin() + b),
                       std::vector<int32_t>(keyPointIndices.begin() + a, keyPointIndices.begin() + b), &cam[4 * k], nKeyPoints[k]);
      out.back().SetRansacParameters(probability, minInliers, maxIterations, minSet, epsilon, th2);
    }
    std::vector<PnPsolver*> ptrs;
    for (PnPsolver& s : out) ptrs.push_back(&s);
    solve_all(ptrs, sets, device);
    return out;
  }

  // :178-271 -> true and Tcw (row-major 4 x 4) when the reference returns a pose: mRefinedTcw of a Refine() with more than
  // minInliers inliers (bNoMore false), or mBestTcw at the mnIterations >= mRansacMaxIts tail (bNoMore true)
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {
    if (!solved_ && !tooFew()) throw std::logic_error("PnPsolver::iterate: call PnPsolver::solve_all first");
    const PnPReplay::Step r = st_.iterate(nIterations, nHyp_, nInliers_.data(), words_.data(), nRec_, recHyp_.data(),
                                          recInliers_.data(), recWords_.data(), kp_.data(), vbInliers);
    bNoMore = r.bNoMore;
    nInliers = r.nInliers;
    const float* v = r.refined >= 0 ? &recPose_[12 * (size_t)r.refined] : (r.best >= 0 ? &pose_[12 * (size_t)r.best] : nullptr);
    if (!v) return false;
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) Tcw[4 * i + j] = v[3 * i + j];
      Tcw[4 * i + 3] = v[9 + i];
    }
    Tcw[12] = Tcw[13] = Tcw[14] = 0.0f; Tcw[15] = 1.0f;
    return true;
  }
  bool find(std::vector<bool>& vbInliers, int& nInliers, float Tcw[16]) {  // :166-170
    bool bFlag;
    return iterate(st_.mRansacMaxIts, bFlag, vbInliers, nInliers, Tcw);
  }

 private:
  std::vector<float> p3d_, p2d_, sigma2_, maxErr_;
  std::vector<int32_t> kp_;
  float cam_[4];
  PnPReplay st_;
  bool solved_ = false;
  int nHyp_ = 0, nRec_ = 0;
  std::vector<int32_t> nInliers_ = {0}, recHyp_ = {0}, recInliers_ = {0};
  std::vector<float> pose_, recPose_;
  std::vector<uint32_t> words_ = {0}, recWords_ = {0};
};

// Initializer (src/Initializer.cc).  keys1 = the reference frame's mvKeysUn points (x y
// interleaved), sigma and iterations as the reference's constructor takes them (:36-43).  FindModels does what Initialize does
// from :57 to :127: compacts vMatches12 into mvMatches12 (:64-73), builds mvSets from the caller's RandomInt values (draws
// [iterations * 8], draws[8 h + j] in [0, N - j); :93-108), evaluates every hypothesis of both models in ONE device call
// (orbfe_initializer_ransac) and replays the two scans (InitializerReplay, orbfe_initializer_replay.hpp).  Reconstruct runs
// ReconstructH / ReconstructF on the chosen model (a second device call and the replay of the tail), and Initialize is both:
// it returns what the reference's Initialize returns, with no reference or OpenCV code on the path.
class Initializer {
 public:
  struct Models {
    double H21[9] = {}, F21[9] = {};   // row-major; meaningful when bestH / bestF >= 0
    int bestH = -1, bestF = -1;        // the hypothesis each scan took, -1: none scored above 0 (an empty cv::Mat)
    double SH = 0.0, SF = 0.0, RH = 0.0;
    bool chooseH = false;              // RH > 0.40 (:127)
    std::vector<bool> vbMatchesInliersH, vbMatchesInliersF;  // indexed like mvMatches12
    std::vector<std::pair<int, int>> mvMatches12;
    std::vector<int32_t> mvSets;       // [iterations * 8]
    std::vector<float> pairs;          // [N * 4] u1 v1 u2 v2 of mvMatches12
    // per (set, model), the layout of orbfe_initializer_ransac
    std::vector<double> score, model, h12;
    std::vector<uint8_t> status;
    std::vector<int32_t> nInliers;
    std::vector<uint32_t> words;
  };

  Initializer(const std::vector<float>& keys1, float sigma = 1.0f, int iterations = 200, int device = 0)
      : keys1_(keys1), sigma_(sigma), iterations_(iterations), device_(device) {
    if (keys1.size() % 2) throw std::invalid_argument("Initializer: keys1 holds x y pairs");
    if (!keys1.empty()) check(orbfe_initializer_normalize((int)(keys1.size() / 2), keys1.data(), T1_), "Initializer");
  }

  Models FindModels(const std::vector<float>& keys2, const std::vector<int>& vMatches12, const std::vector<int32_t>& draws) const {
    if (keys2.size() % 2 || vMatches12.size() != keys1_.size() / 2)
      throw std::invalid_argument("Initializer::FindModels: keys2 holds x y pairs, vMatches12 one entry per reference key");
    if (draws.size() != (size_t)iterations_ * 8) throw std::invalid_argument("Initializer::FindModels: draws holds iterations * 8 values");
    Models m;
    std::vector<float> pairs;
    for (size_t i = 0; i < vMatches12.size(); i++)  // :64-73
      if (vMatches12[i] >= 0) {
        if ((size_t)vMatches12[i] >= keys2.size() / 2) throw std::invalid_argument("Initializer::FindModels: a match outside keys2");
        m.mvMatches12.emplace_back((int)i, vMatches12[i]);
        pairs.insert(pairs.end(), {keys1_[2 * i], keys1_[2 * i + 1], keys2[2 * (size_t)vMatches12[i]], keys2[2 * (size_t)vMatches12[i] + 1]});
      }
    const int N = (int)m.mvMatches12.size(), H = iterations_;
    m.mvSets.assign((size_t)H * 8, 0);
    check(orbfe_initializer_sets_from_draws(N, H, draws.data(), m.mvSets.data()), "Initializer::FindModels");
    double T2[4];
    check(orbfe_initializer_normalize((int)(keys2.size() / 2), keys2.data(), T2), "Initializer::FindModels");  // :150: all keys
    const size_t w = (size_t)((N + 31) / 32);
    m.score.assign((size_t)H * 2, 0.0); m.model.assign((size_t)H * 18, 0.0); m.h12.assign((size_t)H * 9, 0.0);
    m.status.assign((size_t)H * 2, 0); m.nInliers.assign((size_t)H * 2, 0); m.words.assign((size_t)H * 2 * w + 1, 0u);
    check(orbfe_initializer_ransac(device_, N, pairs.data(), T1_, T2, sigma_, H, m.mvSets.data(), m.score.data(), m.status.data(),
                                   m.nInliers.data(), m.model.data(), m.h12.data(), m.words.data()),
          "Initializer::FindModels");
    m.words.resize((size_t)H * 2 * w);
    const InitializerReplay::Pick pH = InitializerReplay::scan(H, ORBFE_INIT_MODEL_H, m.score.data());
    const InitializerReplay::Pick pF = InitializerReplay::scan(H, ORBFE_INIT_MODEL_F, m.score.data());
    m.bestH = pH.best; m.SH = pH.score; m.bestF = pF.best; m.SF = pF.score;
    if (pH.best >= 0) std::memcpy(m.H21, &m.model[9 * (2 * (size_t)pH.best + ORBFE_INIT_MODEL_H)], sizeof m.H21);
    if (pF.best >= 0) std::memcpy(m.F21, &m.model[9 * (2 * (size_t)pF.best + ORBFE_INIT_MODEL_F)], sizeof m.F21);
    InitializerReplay::inliers(N, pH.best, ORBFE_INIT_MODEL_H, m.words.data(), m.vbMatchesInliersH);
    InitializerReplay::inliers(N, pF.best, ORBFE_INIT_MODEL_F, m.words.data(), m.vbMatchesInliersF);
    m.RH = InitializerReplay::ratio(m.SH, m.SF);  // :124
    m.chooseH = InitializerReplay::choose_h(m.RH);
    m.pairs = std::move(pairs);
    return m;
  }

  // What Initialize returns (:52-53), and the device's per-hypothesis results of orbfe_initializer_reconstruct.
  struct Reconstruction {
    bool success = false;
    double R21[9] = {}, t21[3] = {};    // row-major / unit; meaningful when success
    std::vector<float> vP3D;            // [n1 * 3], indexed by the reference key (vMatches12[i].first)
    std::vector<bool> vbTriangulated;   // [n1]
    double parallax = 0.0;              // of the hypothesis taken, degrees
    int modelKind = ORBFE_INIT_MODEL_F, best = -1;
    int nHyp = 0, nInliers = 0;
    uint8_t problemStatus = ORBFE_RECON_PROBLEM_OK;
    std::vector<double> R, t, cosSel, x3d;
    std::vector<int32_t> nGood;
    std::vector<uint8_t> hypStatus, pairFlags;
  };

  // ReconstructH or ReconstructF (:129-131) on the model FindModels chose: ONE device call for the 8 or 4 hypotheses
  // (orbfe_initializer_reconstruct), then the replay of the tail (InitializerReplay::reconstruct_h / _f).  K4 = fx fy cx cy.
  Reconstruction Reconstruct(const Models& m, const float K4[4], double minParallax = 1.0, int minTriangulated = 50) const {
    Reconstruction r;
    const size_t n1 = keys1_.size() / 2, N = m.mvMatches12.size();
    r.vP3D.assign(n1 * 3, 0.0f);
    r.vbTriangulated.assign(n1, false);
    r.modelKind = m.chooseH ? ORBFE_INIT_MODEL_H : ORBFE_INIT_MODEL_F;
    if ((m.chooseH ? m.bestH : m.bestF) < 0) return r;  // an empty model: nothing to reconstruct
    r.nHyp = m.chooseH ? 8 : 4;
    const size_t G = (size_t)r.nHyp;
    std::vector<uint32_t> words;
    InitializerReplay::pack(m.chooseH ? m.vbMatchesInliersH : m.vbMatchesInliersF, words);
    words.push_back(0u);  // (never empty)
    r.R.assign(G * 9, 0.0); r.t.assign(G * 3, 0.0); r.cosSel.assign(G, 0.0); r.nGood.assign(G, 0); r.hypStatus.assign(G, 0);
    r.x3d.assign(G * N * 3 + 1, 0.0); r.pairFlags.assign(G * N + 1, 0);
    int32_t nInl = 0;
    check(orbfe_initializer_reconstruct(device_, (int)N, m.pairs.data(), r.modelKind, m.chooseH ? m.H21 : m.F21, K4, sigma_, words.data(),
                                        r.R.data(), r.t.data(), r.nGood.data(), r.cosSel.data(), r.hypStatus.data(), r.x3d.data(),
                                        r.pairFlags.data(), &r.problemStatus, &nInl),
          "Initializer::Reconstruct");
    r.x3d.resize(G * N * 3); r.pairFlags.resize(G * N);
    r.nInliers = nInl;
    if (r.problemStatus == ORBFE_RECON_DEGENERATE) return r;  // :684-687
    double par[8];
    for (size_t g = 0; g < G; g++) par[g] = InitializerReplay::parallax_degrees(r.nGood[g], r.cosSel[g]);
    const InitializerReplay::Outcome o = m.chooseH ? InitializerReplay::reconstruct_h(nInl, r.nGood.data(), par, minParallax, minTriangulated)
                                                   : InitializerReplay::reconstruct_f(nInl, r.nGood.data(), par, minParallax, minTriangulated);
    if (!o.success) return r;
    r.success = true; r.best = o.best; r.parallax = par[o.best];
    std::memcpy(r.R21, &r.R[9 * (size_t)o.best], sizeof r.R21);
    std::memcpy(r.t21, &r.t[3 * (size_t)o.best], sizeof r.t21);
    for (size_t i = 0; i < N; i++) {
      const size_t s = (size_t)o.best * N + i, first = (size_t)m.mvMatches12[i].first;
      if (r.pairFlags[s] & 1)  // :1011
        for (int c = 0; c < 3; c++) r.vP3D[3 * first + (size_t)c] = (float)r.x3d[3 * s + (size_t)c];
      r.vbTriangulated[first] = (r.pairFlags[s] & 2) != 0;  // :1014-1015
    }
    return r;
  }

  // Initializer::Initialize (:52-135): FindModels + Reconstruct on the chosen model
  bool Initialize(const std::vector<float>& keys2, const std::vector<int>& vMatches12, const std::vector<int32_t>& draws,
                  const float K4[4], double R21[9], double t21[3], std::vector<float>& vP3D, std::vector<bool>& vbTriangulated) const {
    const Reconstruction r = Reconstruct(FindModels(keys2, vMatches12, draws), K4);
    std::memcpy(R21, r.R21, sizeof r.R21);
    std::memcpy(t21, r.t21, sizeof r.t21);
    vP3D = r.vP3D;
    vbTriangulated = r.vbTriangulated;
    return r.success;
  }

 private:
  std::vector<float> keys1_;
  float sigma_;
  int iterations_, device_;
  double T1_[4] = {1.0, 1.0, 0.0, 0.0};
};

// void Frame::ComputeStereoMatches(): fills mvuRight / mvDepth
inline int ComputeStereoMatches(ORBextractor& left, ORBextractor& right, const std::vector<KeyPoint>& kL,
                                const std::vector<uint8_t>& dL, const std::vector<KeyPoint>& kR,
                                const std::vector<uint8_t>& dR, float mbf, float mb, std::vector<float>& mvuRight,
                                std::vector<float>& mvDepth) {
  mvuRight.assign(kL.size(), -1.0f);
  mvDepth.assign(kL.size(), -1.0f);
  int rc = orbfe_compute_stereo_matches(left.handle(), 0, right.handle(), 0,
                                        reinterpret_cast<const orbfe_keypoint*>(kL.data()), dL.data(), (int)kL.size(),
                                        reinterpret_cast<const orbfe_keypoint*>(kR.data()), dR.data(), (int)kR.size(),
                                        mbf, mb, mvuRight.data(), mvDepth.data());
  check(rc, "ComputeStereoMatches");
  return rc;
}

}  // namespace orbfe_cpp
