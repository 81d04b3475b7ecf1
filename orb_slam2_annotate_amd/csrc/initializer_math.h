// initializer_math.h -- one RANSAC hypothesis of Initializer::FindHomography / FindFundamental (src/Initializer.cc:141-255):
// the normalised 8-point DLT of ComputeH21 (:260-305) / ComputeF21 (:307-345) and the per-pair tests of CheckHomography
// (:350-436) / CheckFundamental (:444-526), written once: k_initializer.hip compiles it for the device,
// tests/cpp/initializer_cpu.cpp and tests/cpp/initializer_host_san.cpp for the host.  Plain C++ without a HIP include.
// Arithmetic is binary64 on inputs widened from float (build with -ffp-contract=off).  The reference computes in CV_32F and
// takes its null vector from cv::SVDecomp, so results agree with it to float rounding and are NOT bit-identical to it: a pair
// within float rounding of a threshold may fall on the other side, and a score differs in its last float digits.
//
// The null vector comes from the one-sided Jacobi iteration of jacobi_math.h on the stacked matrix [A; V].  The matrix is held
// BY ROWS, one row of 9 doubles per owner: the device gives every lane of a wave one row (lanes 0-15 the rows of A, lanes
// 16-24 the rows of V), the host programs hold all 25.  `Lanes` says who owns what and how a sum over the rows of A and a
// broadcast are made; the arithmetic, the order of the additions included (a fixed xor butterfly), is the same.
//   * A has 16 rows.  For F only 8 are data and the other 8 are zero, which adds +0.0 to every sum: one code path, two models.
//   * the 36 pairs of a sweep are unrolled, so every column index is a compile-time constant;
//   * the null vector is the column of V under the column of A with the smallest squared norm (the first of equal ones).
//
// IEEE semantics the reference relies on are kept.  cv::Mat::inv() of a singular 3 x 3 matrix (determinant == 0) is the zero
// matrix; with H12 = 0 the projection divides by zero (:398), chiSquare is NaN, `chiSquare > th` is false and the else branch
// adds NaN to the score.  The same happens here; such a hypothesis is kInitNonfinite, and `NaN > score` never selects it.
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#include "jacobi_math.h"  // the one-sided iteration; g2o_mul3, g2o_transpose3, ORBFE_HD of g2o_math.h

namespace orbfe {

enum InitStatus { kInitOk = 0, kInitNonfinite = 1 };  // ORBFE_INIT_* of include/orbfe.h
enum InitModel { kInitH = 0, kInitF = 1 };            // ORBFE_INIT_MODEL_*

constexpr int kInitARows = 16;   // rows of A (lanes 0-15)
constexpr int kInitRows = 25;    // rows of [A; V] (V: lanes 16-24)
constexpr double kInitThH = 5.991;       // :378
constexpr double kInitThF = 3.841;       // :462
constexpr double kInitThScoreF = 5.991;  // :463

// a problem (one Initializer::Initialize) of a call: where its pairs, sets and mask words begin.  Laid out by
// initializer_host.h, read by k_initializer.hip
struct InitProblem {
  int pair0, nPairs;  // pairs [pair0, pair0 + nPairs)
  int hyp0;           // its first set
  int word0, words;   // mask words of its first (set, model); words per (set, model) = ceil(nPairs / 32)
  float sigma;
  double T1[4], T2[4];  // sX sY meanX meanY of Normalize (:852-904)
};

// the host's Lanes: all 25 rows in one place
struct InitHostLanes {
  static constexpr int kOwned = kInitRows;
  int row(int r) const { return r; }
  // the sum over the 16 rows of A as the xor butterfly 8, 4, 2, 1 leaves it in row 0
  double sum_a(const double* part) const {
    double x[kInitARows], y[kInitARows];
    for (int i = 0; i < kInitARows; i++) x[i] = part[i];
    for (int k = kInitARows / 2; k >= 1; k >>= 1) {
      for (int i = 0; i < kInitARows; i++) y[i] = x[i] + x[i ^ k];
      for (int i = 0; i < kInitARows; i++) x[i] = y[i];
    }
    return x[0];
  }
  double pick(const double* vals, int row) const { return vals[row]; }
};

// the sum of 64 per-lane partial scores as the xor butterfly 32, 16, ..., 1 leaves it in lane 0 (the host's form of the
// kernel's shuffle tree)
inline double init_sum64_host(const double* part) {
  double x[64], y[64];
  for (int i = 0; i < 64; i++) x[i] = part[i];
  for (int k = 32; k >= 1; k >>= 1) {
    for (int i = 0; i < 64; i++) y[i] = x[i] + x[i ^ k];
    for (int i = 0; i < 64; i++) x[i] = y[i];
  }
  return x[0];
}

// which of the 8 selected pairs row `id` of [A; V] is built from: ComputeH21 makes rows 2 i, 2 i + 1 from pair i (:268-295),
// ComputeF21 row i (:313-329); -1: a zero row of A or a row of V
ORBFE_HD inline int init_row_pair(int model, int id) {
  if (id >= kInitARows) return -1;
  if (model == kInitH) return id >> 1;
  return id < 8 ? id : -1;
}

// row `id` of [A; V] from its pair p = (u1 v1 u2 v2), normalised as Normalize does: (x - mean) * s
ORBFE_HD inline void init_fill_row(int model, int id, const float p[4], const double T1[4], const double T2[4], double row[9]) {
#pragma unroll
  for (int c = 0; c < 9; c++) row[c] = (id - kInitARows == c) ? 1.0 : 0.0;  // V = I
  if (init_row_pair(model, id) < 0) return;
  const double u1 = ((double)p[0] - T1[2]) * T1[0], v1 = ((double)p[1] - T1[3]) * T1[1];  // :878-896
  const double u2 = ((double)p[2] - T2[2]) * T2[0], v2 = ((double)p[3] - T2[3]) * T2[1];
  if (model == kInitH) {
    const bool odd = (id & 1) != 0;
    row[0] = odd ? u1 : 0.0;  row[1] = odd ? v1 : 0.0;  row[2] = odd ? 1.0 : 0.0;           // :275-277, :285-287
    row[3] = odd ? 0.0 : -u1; row[4] = odd ? 0.0 : -v1; row[5] = odd ? 0.0 : -1.0;          // :278-280, :288-290
    row[6] = odd ? -u2 * u1 : v2 * u1; row[7] = odd ? -u2 * v1 : v2 * v1; row[8] = odd ? -u2 : v2;  // :281-283, :291-293
  } else {
    row[0] = u2 * u1; row[1] = u2 * v1; row[2] = u2;  // :320-328
    row[3] = v2 * u1; row[4] = v2 * v1; row[5] = v2;
    row[6] = u1; row[7] = v1; row[8] = 1.0;
  }
}

// The right singular vector of the smallest singular value of A (the rows of m owned by rows 0-15; rows 16-24 hold V = I on
// entry; m is destroyed): stands where the reference has vt.row(8) of cv::SVDecomp (:301-304, :334-336).  The sign is free:
// it scales H (which cancels in the projections) and F (which cancels in num^2 / (a^2 + b^2)).  Every owner runs the same
// control flow: the sums and hence c, s and whether a pair rotates are the same for all.
template <class L>
ORBFE_HD inline void init_null_vector(const L& ln, double (*m)[9], double nv[9]) {
  const JacobiLaneRows<L, 9> rows = {ln, m};
  jacobi_sweeps_unrolled<9>([&](int p, int q) { return jacobi_cols_pair(rows, p, q); }, JacobiOwnDone());
  double best = 0.0;
#pragma unroll
  for (int j = 0; j < 9; j++) {
    double col[L::kOwned];
#pragma unroll
    for (int r = 0; r < L::kOwned; r++) col[r] = m[r][j];
    const double n2 = rows.dot(j, j);
    if (j == 0 || n2 < best) {
      best = n2;
#pragma unroll
      for (int i = 0; i < 9; i++) nv[i] = ln.pick(col, kInitARows + i);
    }
  }
}

// T of Normalize (:899-903)
ORBFE_HD inline void init_T(const double t[4], double T[9]) {
  T[0] = t[0]; T[1] = 0.0;  T[2] = -t[2] * t[0];
  T[3] = 0.0;  T[4] = t[1]; T[5] = -t[3] * t[1];
  T[6] = 0.0;  T[7] = 0.0;  T[8] = 1.0;
}

// cv::Mat::inv() of a 3 x 3 matrix (DECOMP_LU, which for 3 x 3 is the adjugate over the determinant): the zero matrix when
// the determinant is exactly 0
ORBFE_HD inline void init_inv3(const double M[9], double I[9]) {
  const double c0 = M[4] * M[8] - M[5] * M[7], c1 = M[5] * M[6] - M[3] * M[8], c2 = M[3] * M[7] - M[4] * M[6];
  const double det = M[0] * c0 + M[1] * c1 + M[2] * c2;
  if (det != 0.0) {
    const double d = 1.0 / det;
    I[0] = c0 * d; I[1] = (M[2] * M[7] - M[1] * M[8]) * d; I[2] = (M[1] * M[5] - M[2] * M[4]) * d;
    I[3] = c1 * d; I[4] = (M[0] * M[8] - M[2] * M[6]) * d; I[5] = (M[2] * M[3] - M[0] * M[5]) * d;
    I[6] = c2 * d; I[7] = (M[1] * M[6] - M[0] * M[7]) * d; I[8] = (M[0] * M[4] - M[1] * M[3]) * d;
  } else {
#pragma unroll
    for (int i = 0; i < 9; i++) I[i] = 0.0;
  }
}

// :187-188: H21 = T2^-1 Hn T1, H12 = H21^-1.  T2^-1 is written out (the reference inverts the float matrix)
ORBFE_HD inline void init_model_h(const double nv[9], const double t1[4], const double t2[4], double H21[9], double H12[9]) {
  double T1[9], T2i[9], tmp[9];
  init_T(t1, T1);
  T2i[0] = 1.0 / t2[0]; T2i[1] = 0.0;         T2i[2] = t2[2];
  T2i[3] = 0.0;         T2i[4] = 1.0 / t2[1]; T2i[5] = t2[3];
  T2i[6] = 0.0;         T2i[7] = 0.0;         T2i[8] = 1.0;
  g2o_mul3(T2i, nv, tmp);
  g2o_mul3(tmp, T1, H21);
  init_inv3(H21, H12);
}

// :339-344: the SVD of Fpre, the smallest singular value set to zero, recomposed.  The one-sided iteration on the columns of
// a = Fpre leaves a = U diag(w), v = V, so that Fpre = sum_j a_j v_j^T; the sum without the column of the smallest norm (the
// first of equal ones) is u diag(w') vt.
ORBFE_HD inline void init_rank2(const double Fpre[9], double Fn[9]) {
  double a[9], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0};
#pragma unroll
  for (int i = 0; i < 9; i++) a[i] = Fpre[i];
  jacobi_cols_fixed<3, 3>(a, v, JacobiOwnDone());
  const JacobiCols<3> m = {a, v, 3};
  const double n0 = m.dot(0, 0), n1 = m.dot(1, 1), n2 = m.dot(2, 2);
  int drop = 0;
  double best = n0;
  if (n1 < best) { best = n1; drop = 1; }
  if (n2 < best) { best = n2; drop = 2; }
  const double k0 = drop == 0 ? 0.0 : 1.0, k1 = drop == 1 ? 0.0 : 1.0, k2 = drop == 2 ? 0.0 : 1.0;
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) {
      double f = 0.0;
      if (k0 != 0.0) f += a[3 * i] * v[3 * j];
      if (k1 != 0.0) f += a[3 * i + 1] * v[3 * j + 1];
      if (k2 != 0.0) f += a[3 * i + 2] * v[3 * j + 2];
      Fn[3 * i + j] = f;
    }
}

// :244: F21 = T2^T Fn T1 with Fn the rank-2 matrix of the null vector
ORBFE_HD inline void init_model_f(const double nv[9], const double t1[4], const double t2[4], double F21[9]) {
  double T1[9], T2[9], T2t[9], Fn[9], tmp[9];
  init_T(t1, T1);
  init_T(t2, T2);
  g2o_transpose3(T2, T2t);
  init_rank2(nv, Fn);
  g2o_mul3(T2t, Fn, tmp);
  g2o_mul3(tmp, T1, F21);
}

// CheckHomography for one pair (:384-432): true = vbMatchesInliers[i]; *score receives the pair's terms in the reference's order
ORBFE_HD inline bool init_check_h(const double h[9], const double hi[9], double invSigmaSquare, const float p[4], double* score) {
  const double u1 = (double)p[0], v1 = (double)p[1], u2 = (double)p[2], v2 = (double)p[3];
  bool bIn = true;
  const double w2in1inv = 1.0 / (hi[6] * u2 + hi[7] * v2 + hi[8]);  // :398
  const double u2in1 = (hi[0] * u2 + hi[1] * v2 + hi[2]) * w2in1inv;
  const double v2in1 = (hi[3] * u2 + hi[4] * v2 + hi[5]) * w2in1inv;
  const double squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);  // :402
  const double chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > kInitThH) bIn = false;  // :408-411
  else *score += kInitThH - chiSquare1;
  const double w1in2inv = 1.0 / (h[6] * u1 + h[7] * v1 + h[8]);  // :416
  const double u1in2 = (h[0] * u1 + h[1] * v1 + h[2]) * w1in2inv;
  const double v1in2 = (h[3] * u1 + h[4] * v1 + h[5]) * w1in2inv;
  const double squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);  // :420
  const double chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > kInitThH) bIn = false;  // :424-427
  else *score += kInitThH - chiSquare2;
  return bIn;
}

// CheckFundamental for one pair (:469-522)
ORBFE_HD inline bool init_check_f(const double f[9], double invSigmaSquare, const float p[4], double* score) {
  const double u1 = (double)p[0], v1 = (double)p[1], u2 = (double)p[2], v2 = (double)p[3];
  bool bIn = true;
  const double a2 = f[0] * u1 + f[1] * v1 + f[2], b2 = f[3] * u1 + f[4] * v1 + f[5], c2 = f[6] * u1 + f[7] * v1 + f[8];  // :484-486
  const double num2 = a2 * u2 + b2 * v2 + c2;
  const double squareDist1 = num2 * num2 / (a2 * a2 + b2 * b2);  // :492
  const double chiSquare1 = squareDist1 * invSigmaSquare;
  if (chiSquare1 > kInitThF) bIn = false;  // :496-499
  else *score += kInitThScoreF - chiSquare1;
  const double a1 = f[0] * u2 + f[3] * v2 + f[6], b1 = f[1] * u2 + f[4] * v2 + f[7], c1 = f[2] * u2 + f[5] * v2 + f[8];  // :504-506
  const double num1 = a1 * u1 + b1 * v1 + c1;
  const double squareDist2 = num1 * num1 / (a1 * a1 + b1 * b1);  // :510
  const double chiSquare2 = squareDist2 * invSigmaSquare;
  if (chiSquare2 > kInitThF) bIn = false;  // :514-517
  else *score += kInitThScoreF - chiSquare2;
  return bIn;
}

// the score or an entry of the model (or of H12) not finite: kInitNonfinite, 0 inliers, an all-zero mask
ORBFE_HD inline bool init_nonfinite(double score, const double model[9], const double h12[9]) {
  bool ok = isfinite(score);
#pragma unroll
  for (int i = 0; i < 9; i++) ok = ok && isfinite(model[i]) && isfinite(h12[i]);
  return !ok;
}

// One (set, model) on the host, row by row and pair by pair as the kernel's lanes do: the very additions of the kernel in
// the kernel's order.  pairs = the problem's [n][4]; set = 8 indices into them; words [ceil(n / 32)].
inline void init_hypothesis_host(int model, const InitProblem& P, const float* pairs, const int32_t* set, double* score,
                                 uint8_t* status, int32_t* nInliers, double out[9], double h12[9], uint32_t* words) {
  static const float kNone[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  double m[kInitRows][9], nv[9];
  for (int r = 0; r < kInitRows; r++) {
    const int j = init_row_pair(model, r);
    init_fill_row(model, r, j >= 0 ? pairs + 4 * (size_t)set[j] : kNone, P.T1, P.T2, m[r]);
  }
  const InitHostLanes ln;
  init_null_vector(ln, m, nv);
  for (int i = 0; i < 9; i++) h12[i] = 0.0;
  if (model == kInitH) init_model_h(nv, P.T1, P.T2, out, h12);
  else init_model_f(nv, P.T1, P.T2, out);
  const double invSigmaSquare = 1.0 / ((double)P.sigma * (double)P.sigma);  // :380
  double part[64];
  for (int l = 0; l < 64; l++) part[l] = 0.0;
  for (int w = 0; w < P.words; w++) words[w] = 0;
  int count = 0;
  for (int i = 0; i < P.nPairs; i++) {
    const float* p = pairs + 4 * (size_t)i;
    const bool in = model == kInitH ? init_check_h(out, h12, invSigmaSquare, p, &part[i & 63])
                                    : init_check_f(out, invSigmaSquare, p, &part[i & 63]);
    if (in) { words[i >> 5] |= 1u << (i & 31); count++; }
  }
  *score = init_sum64_host(part);
  const bool bad = init_nonfinite(*score, out, h12);
  if (bad) {
    count = 0;
    for (int w = 0; w < P.words; w++) words[w] = 0;
  }
  *nInliers = count;
  *status = (uint8_t)(bad ? kInitNonfinite : kInitOk);
}

}  // namespace orbfe
