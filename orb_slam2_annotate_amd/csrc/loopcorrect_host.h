// loopcorrect_host.h -- the host arithmetic of the loop correction (include/orbfe.h: orbfe_correct_loop_sim3s,
// orbfe_correct_loop_points, orbfe_gba_propagate_keyframes, orbfe_gba_update_points; device side: loopcorrect.hip,
// k_loopcorrect.hip).  Plain C++ without a HIP include; the kernels take lc_gba_move from here.
// References: LoopClosing::CorrectLoop (src/LoopClosing.cc:514-604) and the tail of
// LoopClosing::RunGlobalBundleAdjustment (src/LoopClosing.cc:787-852).
//
// The float cv::Mat products.  `A * B` of two CV_32F matrices is a cv::MatExpr that cv::gemm evaluates, and
// `R * P + t` is folded by MatExpr into ONE gemm with beta = 1 (modules/core/src/matop.cpp: MatOp_GEMM::add;
// modules/core/src/matmul.cpp: GEMMSingleMul<float, double> -- the accumulator type of CV_32F is double).  The definition
// used here is therefore
//   D_ij = (float)( (double)A_i0 * B_0j + (double)A_i1 * B_1j + ... [+ (double)C_ij] ),  added left to right.
// The product of two binary32 values is exact in binary64, so contraction to FMA cannot change a bit.  No copy of
// matmul.cpp was at hand to check its hand-unrolled path for inner lengths 2 .. 4 against this.
#pragma once
#include <math.h>
#include <stdint.h>

#include <vector>

#include "essgraph_math.h"

namespace orbfe {

// D = A B, 4 x 4 row-major floats
inline void lc_mul44(const float* A, const float* B, float* D) {
  for (int i = 0; i < 4; i++)
    for (int j = 0; j < 4; j++) {
      double s = (double)A[4 * i] * (double)B[j];
      s += (double)A[4 * i + 1] * (double)B[4 + j];
      s += (double)A[4 * i + 2] * (double)B[8 + j];
      s += (double)A[4 * i + 3] * (double)B[12 + j];
      D[4 * i + j] = (float)s;
    }
}

// o = R X + t with R, t the upper 3 x 4 of the row-major 4 x 4 T: one gemm with beta = 1
ORBFE_HD inline void lc_rigid_map(const float* T, const float X[3], float o[3]) {
#pragma unroll
  for (int i = 0; i < 3; i++) {
    double s = (double)T[4 * i] * (double)X[0];
    s += (double)T[4 * i + 1] * (double)X[1];
    s += (double)T[4 * i + 2] * (double)X[2];
    s += (double)T[4 * i + 3];
    o[i] = (float)s;
  }
}

// (:841-850): through the reference key frame's pose before and after the global bundle adjustment
ORBFE_HD inline void lc_gba_move(const float* TcwBef, const float* TwcNew, const float P[3], float out[3]) {
  float Xc[3];
  lc_rigid_map(TcwBef, P, Xc);
  lc_rigid_map(TwcNew, Xc, out);
}

// g2o::Sim3(Converter::toMatrix3d(R), Converter::toVector3d(t), 1.0) of the float pose T (:539-541, :547-549)
inline void lc_sim3_of_pose(const float* T, OptSim3* S) {
  double R[9];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[3 * r + c] = (double)T[4 * r + c];
    S->t[r] = (double)T[4 * r + 3];
  }
  g2o_quat_from_R(R, S->q);
  S->s = 1.0;
}

template <typename T>
inline bool lc_finite(const T* v, size_t n) {
  for (size_t i = 0; i < n; i++)
    if (!isfinite((double)v[i])) return false;
  return true;
}

// what makes K records usable: finite, scale > 0
inline const char* lc_check_records(int K, const double* rec) {
  if (!lc_finite(rec, 8 * (size_t)K)) return "a Sim3 record is not finite";
  for (int k = 0; k < K; k++)
    if (!(rec[8 * (size_t)k + 7] > 0.0)) return "a Sim3 scale is not above 0";
  return nullptr;
}

// (:519-551, :590-596).  NULL when done, else what is wrong (nothing written)
inline const char* correct_loop_sim3s(int K, const float* Tiw, const float* TwcCur, int cur, const double* Scw, double* corrected,
                                      double* noncorrected, float* TiwCorrected) {
  if (K < 1) return "K must be at least 1";
  if (!Tiw || !TwcCur || !Scw || !corrected || !noncorrected || !TiwCorrected) return "NULL argument";
  if (cur < 0 || cur >= K) return "cur outside [0, K)";
  if (!lc_finite(Tiw, 16 * (size_t)K) || !lc_finite(TwcCur, 16)) return "a pose is not finite";
  if (const char* e = lc_check_records(1, Scw)) return e;
  OptSim3 scw;
  ess_load(Scw, &scw);
  for (int k = 0; k < K; k++) {
    const float* T = Tiw + 16 * (size_t)k;
    double* c = corrected + 8 * (size_t)k;
    if (k == cur) {
      for (int i = 0; i < 8; i++) c[i] = Scw[i];  // CorrectedSim3[mpCurrentKF] = mg2oScw (:519)
    } else {
      float Tic[16];
      lc_mul44(T, TwcCur, Tic);  // Tic = Tiw * Twc (:538)
      OptSim3 sic, siw;
      lc_sim3_of_pose(Tic, &sic);
      optsim3_mul(sic, scw, &siw);  // g2oSic * mg2oScw (:542)
      ess_store(siw, c);
    }
    OptSim3 non;
    lc_sim3_of_pose(T, &non);  // (:547-551)
    ess_store(non, noncorrected + 8 * (size_t)k);
    ess_Tiw(c, TiwCorrected + 16 * (size_t)k);  // (:590-596)
  }
  return nullptr;
}

// the claim of (:558-587) on arrays: the lowest k whose list names the point
inline const char* correct_loop_points(int K, const double* corrected, const double* noncorrected, const int32_t* offsets,
                                       const int32_t* point, int n, const float* xw, const uint8_t* skip, float* xwOut,
                                       int32_t* correctedRef) {
  if (K < 0 || n < 0) return "negative count";
  if (!offsets) return "NULL offsets";
  if (K > 0 && (!corrected || !noncorrected)) return "NULL records";
  if (n > 0 && (!xw || !xwOut || !correctedRef)) return "NULL point array";
  if (offsets[0] != 0) return "offsets[0] must be 0";
  for (int k = 0; k < K; k++)
    if (offsets[k + 1] < offsets[k]) return "offsets must not descend";
  if (offsets[K] > 0 && !point) return "NULL point list";
  for (int e = 0; e < offsets[K]; e++)
    if (point[e] < -1 || point[e] >= n) return "point index outside [-1, n_points)";
  if (const char* e = lc_check_records(K, corrected)) return e;
  if (const char* e = lc_check_records(K, noncorrected)) return e;
  for (int p = 0; p < n; p++) {
    correctedRef[p] = -1;
    xwOut[3 * (size_t)p] = xw[3 * (size_t)p]; xwOut[3 * (size_t)p + 1] = xw[3 * (size_t)p + 1]; xwOut[3 * (size_t)p + 2] = xw[3 * (size_t)p + 2];
  }
  for (int k = 0; k < K; k++)
    for (int e = offsets[k]; e < offsets[k + 1]; e++) {
      const int p = point[e];
      if (p < 0 || (skip && skip[p]) || correctedRef[p] >= 0) continue;  // !pMPi, isBad() / mnCorrectedByKF (:570-575)
      ess_correct_point(noncorrected + 8 * (size_t)k, corrected + 8 * (size_t)k, xw + 3 * (size_t)p, xwOut + 3 * (size_t)p);
      correctedRef[p] = k;
    }
  return nullptr;
}

// (:788-815) on indices.  A child's result depends on its parent alone, so the order of the children is immaterial.
inline const char* gba_propagate_keyframes(int n, int nOrigins, const int32_t* origin, const int32_t* childOffsets, const int32_t* child,
                                           const float* Tcw, const float* Twc, const uint8_t* inGba, const float* TcwGba, float* TcwNew,
                                           uint8_t* reached, uint8_t* visited) {
  if (n < 0 || nOrigins < 0) return "negative count";
  if (n == 0) return nOrigins ? "an origin without key frames" : nullptr;
  if (!childOffsets || !Tcw || !Twc || !inGba || !TcwGba || !TcwNew || !reached || !visited || (nOrigins > 0 && !origin)) return "NULL argument";
  if (childOffsets[0] != 0) return "child_offsets[0] must be 0";
  for (int k = 0; k < n; k++)
    if (childOffsets[k + 1] < childOffsets[k]) return "child_offsets must not descend";
  if (childOffsets[n] > 0 && !child) return "NULL child list";
  for (int e = 0; e < childOffsets[n]; e++)
    if (child[e] < 0 || child[e] >= n) return "child index outside [0, n)";
  for (int o = 0; o < nOrigins; o++)
    if (origin[o] < 0 || origin[o] >= n) return "origin index outside [0, n)";
  if (!lc_finite(Tcw, 16 * (size_t)n) || !lc_finite(Twc, 16 * (size_t)n)) return "a pose is not finite";
  for (int k = 0; k < n; k++)
    if (inGba[k] && !lc_finite(TcwGba + 16 * (size_t)k, 16)) return "a pose is not finite";
  for (int o = 0; o < nOrigins; o++)  // an origin's mTcwGBA is applied whatever its flag says (:813)
    if (!lc_finite(TcwGba + 16 * (size_t)origin[o], 16)) return "a pose is not finite";
  // the walk on scratch: nothing is written before it is known to end
  std::vector<float> T(TcwGba, TcwGba + 16 * (size_t)n);
  std::vector<uint8_t> r((size_t)n), v((size_t)n, 0);
  for (int k = 0; k < n; k++) r[(size_t)k] = inGba[k] ? 1 : 0;
  std::vector<int32_t> queue(origin, origin + nOrigins);
  for (int o = 0; o < nOrigins; o++) {
    if (v[(size_t)origin[o]]) return "a key frame is visited twice";
    v[(size_t)origin[o]] = 1;
  }
  for (size_t at = 0; at < queue.size(); at++) {
    const int k = queue[at];
    for (int e = childOffsets[k]; e < childOffsets[k + 1]; e++) {
      const int c = child[e];
      if (v[(size_t)c]) return "a key frame is visited twice (a cycle, or two parents)";
      v[(size_t)c] = 1;
      if (!r[(size_t)c]) {  // pChild->mnBAGlobalForKF != nLoopKF (:801)
        float Tchildc[16];
        lc_mul44(Tcw + 16 * (size_t)c, Twc + 16 * (size_t)k, Tchildc);         // pChild->GetPose() * Twc (:803)
        lc_mul44(Tchildc, T.data() + 16 * (size_t)k, T.data() + 16 * (size_t)c);  // Tchildc * pKF->mTcwGBA (:805)
        r[(size_t)c] = 1;
      }
      queue.push_back(c);
    }
  }
  for (int k = 0; k < n; k++) {
    reached[k] = r[(size_t)k];
    visited[k] = v[(size_t)k];
    for (int i = 0; i < 16; i++) TcwNew[16 * (size_t)k + i] = r[(size_t)k] || v[(size_t)k] ? T[16 * (size_t)k + i] : Tcw[16 * (size_t)k + i];
  }
  return nullptr;
}

// (:818-852) on arrays.  moved: 0 skipped, 1 took mPosGBA, 2 moved through its reference key frame
inline const char* gba_update_points(int p, const float* xw, const uint8_t* bad, const uint8_t* inGba, const float* posGba,
                                     const int32_t* refKf, int nKf, const uint8_t* reached, const float* TcwBef, const float* TwcNew,
                                     float* xwOut, uint8_t* moved) {
  if (p < 0 || nKf < 0) return "negative count";
  if (p == 0) return nullptr;
  if (!xw || !bad || !inGba || !posGba || !refKf || !xwOut || !moved) return "NULL point array";
  if (nKf > 0 && (!reached || !TcwBef || !TwcNew)) return "NULL key-frame array";
  for (int i = 0; i < p; i++)
    if (refKf[i] < -1 || refKf[i] >= nKf) return "ref_kf outside [-1, n_kf)";
  for (int k = 0; k < nKf; k++)
    if (reached[k] && (!lc_finite(TcwBef + 16 * (size_t)k, 16) || !lc_finite(TwcNew + 16 * (size_t)k, 16))) return "a pose is not finite";
  for (int i = 0; i < p; i++) {
    const float* P = xw + 3 * (size_t)i;
    float* o = xwOut + 3 * (size_t)i;
    o[0] = P[0]; o[1] = P[1]; o[2] = P[2];
    moved[i] = 0;
    if (bad[i]) continue;  // (:824)
    if (inGba[i]) {        // (:827-831)
      o[0] = posGba[3 * (size_t)i]; o[1] = posGba[3 * (size_t)i + 1]; o[2] = posGba[3 * (size_t)i + 2];
      moved[i] = 1;
      continue;
    }
    const int r = refKf[i];
    if (r < 0 || !reached[r]) continue;  // (:837); r < 0: the reference would dereference NULL
    lc_gba_move(TcwBef + 16 * (size_t)r, TwcNew + 16 * (size_t)r, P, o);
    moved[i] = 2;
  }
  return nullptr;
}

}  // namespace orbfe
