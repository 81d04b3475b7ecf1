// jacobi_math.h -- the Jacobi iterations that stand where the reference calls cv::SVD, cv::SVDecomp, cv::eigen, cvSVD and
// cvSolve(CV_SVD), written once: the null vectors of the triangulation and of the Initializer's DLT, the 3 x 3 SVDs of the
// Initializer and of PnP, Horn's 4 x 4 eigenvector of Sim3Solver, and the 6 x m least squares and the 12 x 12 eigenvectors of
// EPnP.  triangulate_math.h, sim3_math.h, initializer_math.h, initializer_reconstruct_math.h and pnp_math.h build on it; the
// kernels compile it for the device, the programs under tests/cpp for the host.  Plain C++ without a HIP include.  Arithmetic is
// binary64 (build with -ffp-contract=off); tests/test_jacobi_pins.py holds every routine to its bits.
//
// The rules, for both families:
//   * the step from (al, be, ga) -- the two squared column norms and the dot product, or a_pp, a_qq, a_pq -- to the rotation:
//     zeta = (be - al) / (2 ga), t = sign(zeta) / (|zeta| + sqrt(1 + zeta^2)), c = 1 / sqrt(1 + t^2), s = c t (jacobi_step);
//   * a sweep visits the pairs (p, q), p < q, row-major: (0,1) (0,2) ... (0,n-1) (1,2) ... (n-2,n-1);
//   * at most kJacobiMaxSweeps sweeps, until a sweep rotates nothing;
//   * a comparison with a NaN is false, so a pair with a NaN in its sums is skipped and the iteration ends.
// One-sided (Hestenes), on the columns of the stacked matrix [A; V] with V = I on entry: what cv::SVDecomp's JacobiSVDImpl_
// does, and it does not square the condition number as an eigen-solve of A^T A would.  A pair is skipped -- its columns count as
// orthogonal -- when |a_p . a_q| <= DBL_EPSILON sqrt(|a_p|^2 |a_q|^2).  It leaves A V = U diag(w) in `a`: |a_j| = w_j.
// Two-sided (cyclic), on a symmetric matrix of which both triangles are kept: a pair is skipped -- the entry counts as zero --
// when |a_pq| <= DBL_EPSILON sqrt(|a_pp a_qq|).  It leaves the eigenvalues on the diagonal and the eigenvectors in the columns
// of V.
//
// Where the matrices live is the caller's: the 3 x 3 and 4 x 4 forms run through jacobi_sweeps_unrolled, after which every
// index is a constant and the matrices stay in registers; the PnP forms run through jacobi_sweeps with run-time indices into the
// wave's LDS.  Every sum adds its terms in the order of the rows, 0 first, except where a Lanes policy says otherwise.
#pragma once
#include <float.h>
#include <math.h>

#include "g2o_math.h"  // ORBFE_HD

namespace orbfe {

constexpr int kJacobiMaxSweeps = 30;

// the end of the sweep loop sees `done` = this sweep rotated nothing.  JacobiOwnDone: each problem for itself.  JacobiWaveDone:
// on the device the loop ends when no lane of the wave rotated anything (a lane that is done rotates nothing in further sweeps,
// so its result does not depend on its neighbours); on the host the "wave" is the one problem.
struct JacobiOwnDone {
  ORBFE_HD bool operator()(bool done) const { return done; }
};
struct JacobiWaveDone {
  ORBFE_HD bool operator()(bool done) const {
#if defined(__HIP_DEVICE_COMPILE__)
    return __all(done);
#else
    return done;
#endif
  }
};

ORBFE_HD inline void jacobi_step(double al, double be, double ga, double* c, double* s, double* t) {
  const double zeta = (be - al) / (2.0 * ga);
  *t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  *c = 1.0 / sqrt(1.0 + *t * *t);
  *s = *c * *t;
}
ORBFE_HD inline void jacobi_rot(double& xp, double& xq, double c, double s) {
  const double mp = xp, mq = xq;
  xp = c * mp - s * mq;
  xq = s * mp + c * mq;
}
ORBFE_HD inline void jacobi_identity(double* v, int n) {
  for (int i = 0; i < n * n; i++) v[i] = 0.0;
  for (int i = 0; i < n; i++) v[(n + 1) * i] = 1.0;
}

// the sweeps over pair(p, q) -> "it rotated".  Unrolled: N is a constant and so is every (p, q) the pair step sees.
template <int N, class Pair, class Done>
ORBFE_HD inline void jacobi_sweeps_unrolled(Pair pair, Done done) {
  for (int sweep = 0; sweep < kJacobiMaxSweeps; sweep++) {
    bool rotated = false;
#pragma unroll
    for (int p = 0; p < N - 1; p++)
#pragma unroll
      for (int q = p + 1; q < N; q++) rotated = pair(p, q) || rotated;
    if (done(!rotated)) break;
  }
}
template <class Pair>
ORBFE_HD inline void jacobi_sweeps(int n, Pair pair) {
  for (int sweep = 0; sweep < kJacobiMaxSweeps; sweep++) {
    bool rotated = false;
    for (int p = 0; p < n - 1; p++)
      for (int q = p + 1; q < n; q++) rotated = pair(p, q) || rotated;
    if (!rotated) break;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// One-sided.  A matrix view M says where [A; V] is and how a sum over the rows of A is made:
//   kRows             rows of A (a constant)
//   a(r, j)           A[r][j]
//   vrows(), v(r, j)  the rows of V that are not among those of A
//   dot(p, q)         a_p . a_q
// JacobiCols: A (ROWS x n) and V (n x n) row-major with row length n, sums left to right.
template <int ROWS>
struct JacobiCols {
  static constexpr int kRows = ROWS;
  double* pa;
  double* pv;
  int n;
  ORBFE_HD double& a(int r, int j) const { return pa[n * r + j]; }
  ORBFE_HD int vrows() const { return n; }
  ORBFE_HD double& v(int r, int j) const { return pv[n * r + j]; }
  ORBFE_HD double dot(int p, int q) const {
    double s = a(0, p) * a(0, q);
#pragma unroll
    for (int r = 1; r < ROWS; r++) s += a(r, p) * a(r, q);
    return s;
  }
};
// JacobiLaneRows: [A; V] held BY ROWS of N, L::kOwned of them here (a lane of a wave owns one row, a host program all); the
// rows of V are among them, and the sums over the rows of A go through L::sum_a (initializer_math.h)
template <class L, int N>
struct JacobiLaneRows {
  static constexpr int kRows = L::kOwned;
  const L& ln;
  double (*m)[N];
  ORBFE_HD double& a(int r, int j) const { return m[r][j]; }
  ORBFE_HD int vrows() const { return 0; }
  ORBFE_HD double& v(int r, int j) const { return m[r][j]; }
  ORBFE_HD double dot(int p, int q) const {
    double part[L::kOwned];
#pragma unroll
    for (int r = 0; r < L::kOwned; r++) part[r] = m[r][p] * m[r][q];
    return ln.sum_a(part);
  }
};

// one Hestenes rotation of the columns p, q of A and V; false: skipped
template <class M>
ORBFE_HD inline bool jacobi_cols_pair(const M& m, int p, int q) {
  const double al = m.dot(p, p), be = m.dot(q, q), ga = m.dot(p, q);
  if (!(fabs(ga) > DBL_EPSILON * sqrt(al * be))) return false;
  double c, s, t;
  jacobi_step(al, be, ga, &c, &s, &t);
#pragma unroll
  for (int r = 0; r < M::kRows; r++) jacobi_rot(m.a(r, p), m.a(r, q), c, s);
  // no unroll pragma: vrows() is run-time for PnP.  In the register forms it is the constant 3 or 4 and the compiler unrolls
  // the loop by itself; the forms depend on that (ScratchSize 0 of k_triangulate / k_init_reconstruct / k_pnp_ransac shows it)
  for (int r = 0; r < m.vrows(); r++) jacobi_rot(m.v(r, p), m.v(r, q), c, s);
  return true;
}
// a (ROWS x N, destroyed) -> A V, v (the identity on entry, which the caller writes as a literal) -> V, in registers
template <int ROWS, int N, class Done>
ORBFE_HD inline void jacobi_cols_fixed(double* a, double* v, Done done) {
  const JacobiCols<ROWS> m = {a, v, N};
  jacobi_sweeps_unrolled<N>([&](int p, int q) { return jacobi_cols_pair(m, p, q); }, done);
}

// The right singular vector of the smallest singular value of the 4 x 4 `a` (row-major; destroyed): the column of V under the
// column of A V with the smallest norm (the first of equal ones)
template <class Done>
ORBFE_HD inline void jacobi_null4(double a[16], double x[4], Done done) {
  double v[16] = {1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0};
  jacobi_cols_fixed<4, 4>(a, v, done);
  const JacobiCols<4> m = {a, v, 4};
  const double n0 = m.dot(0, 0), n1 = m.dot(1, 1), n2 = m.dot(2, 2), n3 = m.dot(3, 3);
  double best = n0;
  x[0] = v[0]; x[1] = v[4]; x[2] = v[8]; x[3] = v[12];
  if (n1 < best) { best = n1; x[0] = v[1]; x[1] = v[5]; x[2] = v[9]; x[3] = v[13]; }
  if (n2 < best) { best = n2; x[0] = v[2]; x[1] = v[6]; x[2] = v[10]; x[3] = v[14]; }
  if (n3 < best) { best = n3; x[0] = v[3]; x[1] = v[7]; x[2] = v[11]; x[3] = v[15]; }
}

// columns p < q of the 3 x 3 a and v, and their squared norms n, change places when column p has the strictly smaller norm
ORBFE_HD inline void jacobi_sort3(double a[9], double v[9], double n[3], int p, int q) {
  if (n[p] < n[q]) {
    const double tn = n[p]; n[p] = n[q]; n[q] = tn;
#pragma unroll
    for (int r = 0; r < 3; r++) {
      const double ta = a[3 * r + p]; a[3 * r + p] = a[3 * r + q]; a[3 * r + q] = ta;
      const double tv = v[3 * r + p]; v[3 * r + p] = v[3 * r + q]; v[3 * r + q] = tv;
    }
  }
}

// A = U diag(w) V^T (all 3 x 3 row-major) with full, proper U and V, w descending:
//   * the columns of a = A V sorted by descending norm (a stable bubble of three compares: equal norms keep their order);
//   * w_i = |a_i|, u_i = a_i / w_i for i = 0, 1;
//   * u_2 = +-(u_0 x u_1), the sign that of (u_0 x u_1) . a_2 (a_2 = A v_2), + when that is 0.  For a matrix of rank 2 a_2 is
//     rounding noise and a_2 / |a_2| would be garbage; with this rule U is orthonormal, A = U diag(w) V^T holds and
//     det(U) det(V) is that of a valid SVD.
// The signs of (u_i, v_i) are free, as in any SVD.
ORBFE_HD inline void jacobi_svd3(const double A[9], double U[9], double w[3], double V[9]) {
  double a[9], v[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, n[3];
#pragma unroll
  for (int i = 0; i < 9; i++) a[i] = A[i];
  jacobi_cols_fixed<3, 3>(a, v, JacobiOwnDone());
  const JacobiCols<3> m = {a, v, 3};
#pragma unroll
  for (int j = 0; j < 3; j++) n[j] = m.dot(j, j);
  jacobi_sort3(a, v, n, 0, 1); jacobi_sort3(a, v, n, 1, 2); jacobi_sort3(a, v, n, 0, 1);
#pragma unroll
  for (int j = 0; j < 3; j++) w[j] = sqrt(n[j]);
  const double u0x = a[0] / w[0], u0y = a[3] / w[0], u0z = a[6] / w[0];
  const double u1x = a[1] / w[1], u1y = a[4] / w[1], u1z = a[7] / w[1];
  const double cx = u0y * u1z - u0z * u1y, cy = u0z * u1x - u0x * u1z, cz = u0x * u1y - u0y * u1x;
  const double dot = cx * a[2] + cy * a[5] + cz * a[8];
  const double sg = dot < 0.0 ? -1.0 : 1.0;
  U[0] = u0x; U[1] = u1x; U[2] = sg * cx;
  U[3] = u0y; U[4] = u1y; U[5] = sg * cy;
  U[6] = u0z; U[7] = u1z; U[8] = sg * cz;
#pragma unroll
  for (int i = 0; i < 9; i++) V[i] = v[i];
}

// ---------------------------------------------------------------------------------------------------------------------
// Two-sided: one rotation of the symmetric n x n `a` (row-major) in the plane (p, q) and of the columns p, q of `v` -- the
// diagonal, the zeroed a_pq, the entries of every other row mirrored into both triangles; false: skipped
ORBFE_HD inline bool jacobi_sym_pair(double* a, double* v, int n, int p, int q) {
  const double apq = a[n * p + q], app = a[(n + 1) * p], aqq = a[(n + 1) * q];
  if (!(fabs(apq) > DBL_EPSILON * sqrt(fabs(app * aqq)))) return false;
  double c, s, t;
  jacobi_step(app, aqq, apq, &c, &s, &t);
  a[(n + 1) * p] = app - t * apq;
  a[(n + 1) * q] = aqq + t * apq;
  a[n * p + q] = a[n * q + p] = 0.0;
  // no unroll pragma, as above: n = 12 stays a loop over LDS, n = 4 (k_sim3) is unrolled by the compiler, which the register
  // form depends on (ScratchSize 0 of k_sim3 shows it)
  for (int r = 0; r < n; r++) {
    if (r != p && r != q) {
      const double rp = a[n * r + p], rq = a[n * r + q];
      a[n * r + p] = a[n * p + r] = c * rp - s * rq;
      a[n * r + q] = a[n * q + r] = s * rp + c * rq;
    }
    jacobi_rot(v[n * r + p], v[n * r + q], c, s);
  }
  return true;
}

}  // namespace orbfe
