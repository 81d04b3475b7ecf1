// OpenCV double for building the REFERENCE's src/ORBextractor.cc untouched (oracle/Makefile, target `ref`).
// Written for this project; it declares only what that file and include/ORBextractor.h name: an 8-bit
// single-channel Mat that shares its buffer between views as cv::Mat does, Point_/Size/Rect/KeyPoint,
// InputArray/OutputArray, and the DECLARATIONS of the OpenCV functions the extractor calls.  Those functions are
// defined in oracle/orbextractor_ref_shim.cpp on top of the oracle's primitives.  Test infrastructure only.
#ifndef ORBFE_REF_CV_CORE_HPP
#define ORBFE_REF_CV_CORE_HPP

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <iterator>
#include <memory>
#include <vector>

typedef unsigned char uchar;

#define CV_8U 0
#define CV_8UC1 0
#define CV_PI 3.1415926535897932384626433832795

int cvRound(double value);
int cvFloor(double value);
int cvCeil(double value);

namespace cv {

enum { INTER_LINEAR = 1 };
enum { BORDER_REFLECT_101 = 4, BORDER_ISOLATED = 16 };

template <typename T> struct Point_ {
  T x, y;
  Point_() : x(0), y(0) {}
  Point_(T _x, T _y) : x(_x), y(_y) {}
  template <typename S> Point_& operator*=(S s) { x = (T)(x * s); y = (T)(y * s); return *this; }
};
typedef Point_<int> Point2i;
typedef Point_<int> Point;
typedef Point_<float> Point2f;

struct Size {
  int width, height;
  Size() : width(0), height(0) {}
  Size(int w, int h) : width(w), height(h) {}
};

struct Rect {
  int x, y, width, height;
  Rect(int _x, int _y, int w, int h) : x(_x), y(_y), width(w), height(h) {}
};

struct Scalar {};

struct KeyPoint {  // 28 bytes, the layout the project's keypoint records share
  Point2f pt;
  float size, angle, response;
  int octave, class_id;
  KeyPoint() : pt(0, 0), size(0), angle(-1), response(0), octave(0), class_id(-1) {}
  KeyPoint(float x, float y, float _size, float _angle = -1, float _response = 0, int _octave = 0, int _class_id = -1)
      : pt(x, y), size(_size), angle(_angle), response(_response), octave(_octave), class_id(_class_id) {}
};

struct MatZeros { int rows, cols; };  // what Mat::zeros returns: assigned INTO a Mat of that size, as a MatExpr is

class Mat {
 public:
  int rows, cols;
  uchar* data;
  size_t step;  // bytes per row of the buffer this view looks into

  Mat() : rows(0), cols(0), data(0), step(0) {}
  Mat(int r, int c, int) { allocate(r, c); }
  Mat(Size sz, int) { allocate(sz.height, sz.width); }

  // create() of an array that already has the size keeps its buffer: the reference relies on it
  void create(int r, int c, int) { if (r != rows || c != cols || !data) allocate(r, c); }
  void release() { buf.reset(); rows = cols = 0; data = 0; step = 0; }
  bool empty() const { return data == 0 || rows * cols == 0; }
  int type() const { return CV_8UC1; }
  size_t step1() const { return step; }
  template <typename T> T& at(int y, int x) { return *(T*)(data + (size_t)y * step + x); }
  template <typename T> const T& at(int y, int x) const { return *(const T*)(data + (size_t)y * step + x); }
  uchar* ptr(int y = 0) { return data + (size_t)y * step; }
  const uchar* ptr(int y = 0) const { return data + (size_t)y * step; }
  Mat rowRange(int a, int b) const { return view(0, a, cols, b - a); }
  Mat colRange(int a, int b) const { return view(a, 0, b - a, rows); }
  Mat operator()(const Rect& r) const { return view(r.x, r.y, r.width, r.height); }
  Mat clone() const {
    Mat m(rows, cols, CV_8UC1);
    for (int y = 0; y < rows; y++) std::memcpy(m.ptr(y), ptr(y), cols);
    return m;
  }
  static MatZeros zeros(int r, int c, int) { MatZeros z = {r, c}; return z; }
  Mat& operator=(const MatZeros& z) {
    create(z.rows, z.cols, CV_8UC1);
    for (int y = 0; y < rows; y++) std::memset(ptr(y), 0, cols);
    return *this;
  }

 private:
  std::shared_ptr<std::vector<uchar> > buf;
  void allocate(int r, int c) {
    buf.reset(new std::vector<uchar>((size_t)r * c));
    rows = r; cols = c; step = (size_t)c; data = buf->empty() ? 0 : &(*buf)[0];
  }
  Mat view(int x, int y, int w, int h) const {
    assert(x >= 0 && y >= 0 && w >= 0 && h >= 0 && x + w <= cols && y + h <= rows);
    Mat m;
    m.buf = buf; m.rows = h; m.cols = w; m.step = step; m.data = data + (size_t)y * step + x;
    return m;
  }
};

class _InputArray {
 public:
  _InputArray(const Mat& m) : mat(const_cast<Mat*>(&m)) {}
  bool empty() const { return mat->empty(); }
  Mat getMat() const { return *mat; }
 protected:
  Mat* mat;
};
class _OutputArray : public _InputArray {
 public:
  _OutputArray(Mat& m) : _InputArray(m) {}
  void release() const { mat->release(); }
  void create(int r, int c, int t) const { mat->create(r, c, t); }
};
typedef const _InputArray& InputArray;
typedef const _OutputArray& OutputArray;

float fastAtan2(float y, float x);
void FAST(InputArray image, std::vector<KeyPoint>& keypoints, int threshold, bool nonmaxSuppression = true);
void GaussianBlur(InputArray src, OutputArray dst, Size ksize, double sigmaX, double sigmaY = 0,
                  int borderType = BORDER_REFLECT_101);
void resize(InputArray src, OutputArray dst, Size dsize, double fx = 0, double fy = 0, int interpolation = INTER_LINEAR);
void copyMakeBorder(InputArray src, OutputArray dst, int top, int bottom, int left, int right, int borderType,
                    const Scalar& value = Scalar());

struct KeyPointsFilter {
  static void retainBest(std::vector<KeyPoint>& keypoints, int npoints);
};

}  // namespace cv

#endif
