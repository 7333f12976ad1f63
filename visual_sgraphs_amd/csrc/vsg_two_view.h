// vsg_two_view.h -- TwoViewReconstruction::Reconstruct (TwoViewReconstruction.cc; Tracking.cc:2568 through
// Pinhole.cpp:91-101), the monocular initialisation, host and device from one source: Normalize (:735-782), ONE RANSAC
// hypothesis of either model (ComputeH21 / ComputeF21, :231-306) with its score (CheckHomography / CheckFundamental,
// :308-471), the selection over the scores that the two loops (:155-178, :205-228) amount to, the motion hypotheses of
// ReconstructF / DecomposeE / ReconstructH (:473-733, :900-925), CheckRT's test of one match (:784-898) and the final
// choice.  The kernels of vsg_two_view.hip run it on the device; tests/_twoviewcore compiles it for the host
// (two_view::reconstruct_host).  As in vsg_sim3.h / vsg_triangulate.h the order is fixed and nothing contracts: every
// operation is one vsg::f* / vsg::d* call = one rounding, every comparison is written as the reference writes it, so that
// a NaN takes the reference's branch.  No libm other than sqrt.
//
// Hypothesis `it` depends on mvSets[it] alone and each loop keeps the first `it` whose score is strictly greater than
// every earlier one: the search is independent work plus a selection, not a sequence.
//
// THE SCORE IS AN ORDERED FLOAT SUM (match 0's first term, its second term, match 1's, ...): `currentScore > score` picks
// the winner, so the order is part of the result.  A term that the reference does not add is added here as +0.0f, which
// leaves a sum that started at +0 and only ever receives values >= +0 (or NaN) unchanged bit for bit.
//
// WHERE THE REFERENCE IS DOUBLE.  invSigmaSquare = 1.0 / (sigma * sigma), w2in1inv = 1.0 / (float), invZ = 1.0 / z, sX =
// 1.0 / meanDevX are double quotients of a float, rounded to float.  0.7 * maxGood, 0.9 * N, 0.75 * bestGood are doubles
// compared with ints; cosParallax < 0.99998 and d1 / d2 < 1.00001 compare a float with a double literal.
//
// DEVIATIONS of arithmetic class, measured by tests/test_two_view_reference.py:
//   1. every singular vector comes from the double one-sided Jacobi of vsg_jacobi.h (a compile-time number of sweeps, a
//      fixed pair order) rounded to float once, where the reference runs Eigen's float JacobiSVD: the ninth right
//      singular vector of the 16 x 9 / 8 x 9 systems, U, w, V of the rank-2 step of F (:300-305), of DecomposeE (:903)
//      and of ReconstructH (:586).  U = the columns of A V divided by their norms, the singular values sorted descending
//      as Eigen leaves them (equal ones keep their order).  The SIGN of a singular pair is free; DESIGN.md shows that it
//      permutes the motion hypotheses among themselves and changes no output other than the order of n_good[].
//   2. Eigen's 3 x 3 inverse (H12i = H21i.inverse(), T2.inverse(), K.inverse()) is restated as cofactors times the
//      reciprocal determinant in the order of Eigen's compute_inverse_size3; products of 3 x 3 matrices sum their three
//      terms left to right.  Eigen's vectorised kernels may associate differently: rounding.
//   3. GeometricTools::Triangulate returns false with x3D UNSET when x3Dh(3) == 0 and CheckRT ignores the return value
//      (:830): undefined in the reference, defined here as "not finite" -- the :832 branch, the match is skipped.
//
// acos IS NOT RESTATED.  The choice among the 4 or 8 motion hypotheses is by nGood alone, so the device picks the
// hypothesis and returns the COSINE of rank min(50, size - 1) (:889-892; a rank count, not a sort -- equal values make the
// choice of element immaterial); the host applies acos(...) * 180 / CV_PI and the parallax gate after the wait
// (two_view::finish).
//
// KEPT QUIRKS (each pinned by a test): Normalize runs over ALL keypoints of a frame, not the matched ones; F gates at
// 3.841 but scores against 5.991; the strict first maximum; a point with cosParallax >= 0.99998 counts in nGood and has
// its position written but is not flagged triangulated (:879-884); the index-50 rule; ReconstructH never assigns vP3D
// (:724-730), so on the H path the caller's x3d is left as it was.
#pragma once
#include <stddef.h>

#include <cmath>
#include <thread>
#include <vector>

#include "../../include/vsg_orb.h"
#include "vsg_frustum.h"
#include "vsg_jacobi.h"
#include "vsg_math.h"
#include "vsg_triangulate.h"

#if defined(__HIPCC__)
#define VSG_TV_UNROLL _Pragma("unroll")
#else
#define VSG_TV_UNROLL
#endif

namespace vsg {
namespace two_view {

// Hestenes sweeps.  Trial (tests/test_two_view_reference.py prints it: this routine on the 16 x 9 and 8 x 9 systems of every
// hypothesis of the sixteen scenes of tests/two_view_scenes.py, 3200 + 3161 matrices, those with a relative gap of the two
// least singular values below 1e-4 left out): against numpy.linalg.svd in double the largest component error of the unit
// null vector was 4.5e-1 / 6.5e-3 / 3.4e-8 / 2.3e-13 (H) and 7.0e-1 / 4.0e-1 / 1.8e-5 / 3.4e-13 (F) after 5 .. 8 sweeps and
// stayed there up to 12 (the conditioning: 1e-16 over the gap).  One more than the 8 it took.  The 3 x 3 decompositions
// (480 essential and homography matrices of those scenes; singular values, orthogonality of U Sigma and of V) were final
// (1.3e-15) after 4; one more.
enum { kSweeps9 = 9, kSweeps3 = 5 };
enum { kMaxIterations = 1024 };
enum { kModelH = 0, kModelF = 1 };
enum { kOk = 0, kNoScore = 1, kSingularValues = 2, kNoWinner = 3, kLowParallax = 4 };

VSG_HD float canonf(float v) { return v != v ? __builtin_nanf("") : v; }
VSG_HD bool finitef(float v) { return fsub(v, v) == 0.0f; }  // isfinite: inf - inf and NaN - NaN are NaN

// T of Normalize (:776-781) by its four numbers: T = [sx 0 -mean_x * sx; 0 sy -mean_y * sy; 0 0 1]
struct Norm {
  float mean_x, mean_y, sx, sy;
};
// one match: the undistorted keypoints (kp1.pt, kp2.pt) and their normalised coordinates (vPn1[first], vPn2[second])
struct Match {
  float u1, v1, u2, v2, x1, y1, x2, y2;
};
struct Motion {
  float R[9], t[3];
};
// what the selection leaves behind for CheckRT and the last step
struct Selected {
  int model, reason, n_motion, n_inliers;  // reason: kOk, kNoScore or kSingularValues
  int best_it_h, best_it_f;                // -1: no hypothesis scored above 0
  float SH, SF, H21[9], F21[9];
  Motion motion[8];
};
// CheckRT's verdict on one match
enum { kRtSkipped = 0, kRtCounted = 1, kRtTriangulated = 2 };

// ---- Normalize (:735-782) over ALL n keypoints, in index order, in float.  xy(i, &x, &y) reads keypoint i.
template <class XY>
inline Norm normalize(int n, XY xy) {
  float meanX = 0, meanY = 0;
  for (int i = 0; i < n; i++) {
    float x, y;
    xy(i, &x, &y);
    meanX = fadd(meanX, x), meanY = fadd(meanY, y);
  }
  meanX = fdiv(meanX, (float)n), meanY = fdiv(meanY, (float)n);
  float meanDevX = 0, meanDevY = 0;
  for (int i = 0; i < n; i++) {
    float x, y;
    xy(i, &x, &y);
    const float dx = fsub(x, meanX), dy = fsub(y, meanY);
    meanDevX = fadd(meanDevX, dx < 0 ? -dx : (dx == 0 ? 0.0f : dx));  // fabs: -0 becomes +0
    meanDevY = fadd(meanDevY, dy < 0 ? -dy : (dy == 0 ? 0.0f : dy));
  }
  meanDevX = fdiv(meanDevX, (float)n), meanDevY = fdiv(meanDevY, (float)n);
  Norm t;
  t.mean_x = meanX, t.mean_y = meanY;
  t.sx = (float)ddiv(1.0, (double)meanDevX), t.sy = (float)ddiv(1.0, (double)meanDevY);
  return t;
}
VSG_HD void norm_matrix(const Norm &n, float *T) {
  T[0] = n.sx, T[1] = 0.0f, T[2] = fmul(-n.mean_x, n.sx);
  T[3] = 0.0f, T[4] = n.sy, T[5] = fmul(-n.mean_y, n.sy);
  T[6] = 0.0f, T[7] = 0.0f, T[8] = 1.0f;
}
VSG_HD Match make_match(const Norm &n1, const Norm &n2, float u1, float v1, float u2, float v2) {
  Match m;
  m.u1 = u1, m.v1 = v1, m.u2 = u2, m.v2 = v2;
  m.x1 = fmul(fsub(u1, n1.mean_x), n1.sx), m.y1 = fmul(fsub(v1, n1.mean_y), n1.sy);  // :757-758, :772-773
  m.x2 = fmul(fsub(u2, n2.mean_x), n2.sx), m.y2 = fmul(fsub(v2, n2.mean_y), n2.sy);
  return m;
}

// ---- 3 x 3 float matrices, row-major
VSG_HD void mul3(const float *A, const float *B, float *C) {
  VSG_TV_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_TV_UNROLL
    for (int j = 0; j < 3; j++) C[3 * i + j] = dot3(A[3 * i], A[3 * i + 1], A[3 * i + 2], B[j], B[3 + j], B[6 + j]);
}
VSG_HD void transpose3(const float *A, float *At) {
  VSG_TV_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_TV_UNROLL
    for (int j = 0; j < 3; j++) At[3 * i + j] = A[3 * j + i];
}
VSG_HD float cofactor3(const float *m, int i1, int i2, int j1, int j2) {
  return fsub(fmul(m[3 * i1 + j1], m[3 * i2 + j2]), fmul(m[3 * i1 + j2], m[3 * i2 + j1]));
}
// the cofactors of column 0, their dot product with column 0 (the determinant), then cofactor^T * (1 / det)
VSG_HD float det3(const float *m) {
  const float c00 = cofactor3(m, 1, 2, 1, 2), c10 = cofactor3(m, 2, 0, 1, 2), c20 = cofactor3(m, 0, 1, 1, 2);
  return fadd(fadd(fmul(c00, m[0]), fmul(c10, m[3])), fmul(c20, m[6]));
}
VSG_HD void inverse3(const float *m, float *inv) {
  const float c00 = cofactor3(m, 1, 2, 1, 2), c10 = cofactor3(m, 2, 0, 1, 2), c20 = cofactor3(m, 0, 1, 1, 2);
  const float det = fadd(fadd(fmul(c00, m[0]), fmul(c10, m[3])), fmul(c20, m[6]));
  const float invdet = fdiv(1.0f, det);
  inv[0] = fmul(c00, invdet), inv[1] = fmul(c10, invdet), inv[2] = fmul(c20, invdet);
  inv[3] = fmul(cofactor3(m, 1, 2, 2, 0), invdet), inv[4] = fmul(cofactor3(m, 2, 0, 2, 0), invdet);
  inv[5] = fmul(cofactor3(m, 0, 1, 2, 0), invdet);
  inv[6] = fmul(cofactor3(m, 1, 2, 0, 1), invdet), inv[7] = fmul(cofactor3(m, 2, 0, 0, 1), invdet);
  inv[8] = fmul(cofactor3(m, 0, 1, 0, 1), invdet);
}

// U, w, V of the float 3 x 3 A (row-major), A = U diag(w) V^T, w descending, in double and rounded once (deviation 1)
VSG_HD void svd3(const float *A, float *U, float *w, float *V) {
  JacobiRegs<3, 3> s;
  VSG_TV_UNROLL
  for (int r = 0; r < 3; r++)
    VSG_TV_UNROLL
    for (int c = 0; c < 3; c++) s.at(r, c) = (double)A[3 * r + c], s.at(3 + r, c) = r == c ? 1.0 : 0.0;
  jacobi_sweeps<3, 3, kSweeps3>(s);
  double sg[3];
  VSG_TV_UNROLL
  for (int c = 0; c < 3; c++) sg[c] = dsqrt(jacobi_column_norm2<3, 3>(s, c));
  // descending, equal values keep their order: three compare-and-swaps on whole columns (selects, no indexing)
  VSG_TV_UNROLL
  for (int step = 0; step < 3; step++) {
    const int a = step == 1 ? 1 : 0, b = a + 1;
    if (sg[a] < sg[b]) {
      const double ts = sg[a];
      sg[a] = sg[b], sg[b] = ts;
      VSG_TV_UNROLL
      for (int r = 0; r < 6; r++) {
        const double tw = s.at(r, a);
        s.at(r, a) = s.at(r, b), s.at(r, b) = tw;
      }
    }
  }
  VSG_TV_UNROLL
  for (int c = 0; c < 3; c++) {
    w[c] = (float)sg[c];
    VSG_TV_UNROLL
    for (int r = 0; r < 3; r++) U[3 * r + c] = (float)ddiv(s.at(r, c), sg[c]), V[3 * r + c] = (float)s.at(3 + r, c);
  }
}

// ---- one hypothesis.  J<M, N> = the Jacobi storage policy built from ctx (vsg_jacobi.h); pt(j, p) = the normalised
// coordinates {x1, y1, x2, y2} of the j-th sampled match.

// ComputeH21 (:231-270): row r of the 16 x 9 float system, as doubles
template <class S, class PT>
VSG_HD void h_row(S &s, int r, PT pt) {
  float p[4];
  pt(r >> 1, p);
  const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
  const bool odd = (r & 1) != 0;
  s.at(r, 0) = odd ? (double)u1 : 0.0, s.at(r, 1) = odd ? (double)v1 : 0.0, s.at(r, 2) = odd ? 1.0 : 0.0;
  s.at(r, 3) = odd ? 0.0 : (double)-u1, s.at(r, 4) = odd ? 0.0 : (double)-v1, s.at(r, 5) = odd ? 0.0 : -1.0;
  s.at(r, 6) = (double)(odd ? fmul(-u2, u1) : fmul(v2, u1));
  s.at(r, 7) = (double)(odd ? fmul(-u2, v1) : fmul(v2, v1));
  s.at(r, 8) = (double)(odd ? -u2 : v2);
}
// ComputeF21 (:272-298): row r of the 8 x 9 system
template <class S, class PT>
VSG_HD void f_row(S &s, int r, PT pt) {
  float p[4];
  pt(r, p);
  const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
  s.at(r, 0) = (double)fmul(u2, u1), s.at(r, 1) = (double)fmul(u2, v1), s.at(r, 2) = (double)u2;
  s.at(r, 3) = (double)fmul(v2, u1), s.at(r, 4) = (double)fmul(v2, v1), s.at(r, 5) = (double)v2;
  s.at(r, 6) = (double)u1, s.at(r, 7) = (double)v1, s.at(r, 8) = 1.0;
}
template <int M, class S>
VSG_HD void null9(S &s, float *v9) {
  jacobi_sweeps<M, 9, kSweeps9>(s);
  double v[9];
  jacobi_null_vector<M, 9>(s, v);
  VSG_TV_UNROLL
  for (int k = 0; k < 9; k++) v9[k] = (float)v[k];
}

// H21i = T2inv * Hn * T1, H12i = H21i.inverse() (:166-168)
template <class S, class PT>
VSG_HD void hypothesis_h(S &s, PT pt, const float *T1, const float *T2inv, float *H21, float *H12) {
  s.rows([&](int r) {
    if (r < 16)
      h_row(s, r, pt);
    else
      jacobi_identity_row<16, 9>(s, r);
  });
  s.sync();
  float Hn[9], tmp[9];
  null9<16>(s, Hn);
  mul3(T2inv, Hn, tmp), mul3(tmp, T1, H21);
  inverse3(H21, H12);
}
// F21i = T2t * Fn * T1 with Fn of rank 2 (:216-218, :300-305)
template <class S, class PT>
VSG_HD void hypothesis_f(S &s, PT pt, const float *T1, const float *T2t, float *F21) {
  s.rows([&](int r) {
    if (r < 8)
      f_row(s, r, pt);
    else
      jacobi_identity_row<8, 9>(s, r);
  });
  s.sync();
  float Fpre[9], U[9], w[3], V[9], Uw[9], Vt[9], Fn[9], tmp[9];
  null9<8>(s, Fpre);
  svd3(Fpre, U, w, V);
  w[2] = 0.0f;
  VSG_TV_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_TV_UNROLL
    for (int j = 0; j < 3; j++) Uw[3 * i + j] = fmul(U[3 * i + j], w[j]);
  transpose3(V, Vt);
  mul3(Uw, Vt, Fn);
  mul3(T2t, Fn, tmp), mul3(tmp, T1, F21);
}

// ---- the two score terms of one match and its inlier flag.  th = 5.991f; invSigmaSquare = (float)(1.0 / (sigma * sigma))
VSG_HD float inv_sigma_square(float sigma) { return (float)ddiv(1.0, (double)fmul(sigma, sigma)); }

VSG_HD bool score_h(const float *H21, const float *H12, const Match &m, float invSigmaSquare, float *t1, float *t2) {
  const float th = 5.991f;
  bool bIn = true;
  const float u1 = m.u1, v1 = m.v1, u2 = m.u2, v2 = m.v2;
  const float w2in1inv = (float)ddiv(1.0, (double)fadd(fadd(fmul(H12[6], u2), fmul(H12[7], v2)), H12[8]));  // :355
  const float u2in1 = fmul(fadd(fadd(fmul(H12[0], u2), fmul(H12[1], v2)), H12[2]), w2in1inv);
  const float v2in1 = fmul(fadd(fadd(fmul(H12[3], u2), fmul(H12[4], v2)), H12[5]), w2in1inv);
  const float du1 = fsub(u1, u2in1), dv1 = fsub(v1, v2in1);
  const float chiSquare1 = fmul(fadd(fmul(du1, du1), fmul(dv1, dv1)), invSigmaSquare);
  if (chiSquare1 > th)
    bIn = false, *t1 = 0.0f;
  else
    *t1 = fsub(th, chiSquare1);
  const float w1in2inv = (float)ddiv(1.0, (double)fadd(fadd(fmul(H21[6], u1), fmul(H21[7], v1)), H21[8]));  // :371
  const float u1in2 = fmul(fadd(fadd(fmul(H21[0], u1), fmul(H21[1], v1)), H21[2]), w1in2inv);
  const float v1in2 = fmul(fadd(fadd(fmul(H21[3], u1), fmul(H21[4], v1)), H21[5]), w1in2inv);
  const float du2 = fsub(u2, u1in2), dv2 = fsub(v2, v1in2);
  const float chiSquare2 = fmul(fadd(fmul(du2, du2), fmul(dv2, dv2)), invSigmaSquare);
  if (chiSquare2 > th)
    bIn = false, *t2 = 0.0f;
  else
    *t2 = fsub(th, chiSquare2);
  return bIn;
}
VSG_HD bool score_f(const float *F, const Match &m, float invSigmaSquare, float *t1, float *t2) {
  const float th = 3.841f, thScore = 5.991f;
  bool bIn = true;
  const float u1 = m.u1, v1 = m.v1, u2 = m.u2, v2 = m.v2;
  const float a2 = fadd(fadd(fmul(F[0], u1), fmul(F[1], v1)), F[2]);  // :431-433
  const float b2 = fadd(fadd(fmul(F[3], u1), fmul(F[4], v1)), F[5]);
  const float c2 = fadd(fadd(fmul(F[6], u1), fmul(F[7], v1)), F[8]);
  const float num2 = fadd(fadd(fmul(a2, u2), fmul(b2, v2)), c2);
  const float squareDist1 = fdiv(fmul(num2, num2), fadd(fmul(a2, a2), fmul(b2, b2)));
  const float chiSquare1 = fmul(squareDist1, invSigmaSquare);
  if (chiSquare1 > th)
    bIn = false, *t1 = 0.0f;
  else
    *t1 = fsub(thScore, chiSquare1);
  const float a1 = fadd(fadd(fmul(F[0], u2), fmul(F[3], v2)), F[6]);  // :449-451
  const float b1 = fadd(fadd(fmul(F[1], u2), fmul(F[4], v2)), F[7]);
  const float c1 = fadd(fadd(fmul(F[2], u2), fmul(F[5], v2)), F[8]);
  const float num1 = fadd(fadd(fmul(a1, u1), fmul(b1, v1)), c1);
  const float squareDist2 = fdiv(fmul(num1, num1), fadd(fmul(a1, a1), fmul(b1, b1)));
  const float chiSquare2 = fmul(squareDist2, invSigmaSquare);
  if (chiSquare2 > th)
    bIn = false, *t2 = 0.0f;
  else
    *t2 = fsub(thScore, chiSquare2);
  return bIn;
}

// ---- the selection of one loop (:155-178 / :205-228) from the scores in order: the first `it` whose score is strictly
// greater than every earlier one, starting from 0.  -1: none (the reference's matrix is then never assigned).  A NaN
// score never wins.
VSG_HD int first_maximum(const float *score, int n_iter) {
  int best = -1;
  float s = 0.0f;
  for (int it = 0; it < n_iter; it++)
    if (score[it] > s) s = score[it], best = it;
  return best;
}

// ---- the motion hypotheses
// DecomposeE (:900-925) of E21 = K^T * F21 * K (:482), then {R1, t}, {R2, t}, {R1, -t}, {R2, -t} (:498-501)
VSG_HD void motions_f(const float *F21, const float *K, Motion *mo) {
  float Kt[9], tmp[9], E[9], U[9], w[3], V[9], Vt[9];
  transpose3(K, Kt);
  mul3(Kt, F21, tmp), mul3(tmp, K, E);
  svd3(E, U, w, V);
  transpose3(V, Vt);
  float t[3] = {U[2], U[5], U[8]};
  const float tn = fsqrt(dot3(t[0], t[1], t[2], t[0], t[1], t[2]));
  VSG_TV_UNROLL
  for (int k = 0; k < 3; k++) t[k] = fdiv(t[k], tn);
  const float W[9] = {0.0f, -1.0f, 0.0f, 1.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f};
  float Wt[9], R1[9], R2[9];
  transpose3(W, Wt);
  mul3(U, W, tmp), mul3(tmp, Vt, R1);
  if (det3(R1) < 0)
    VSG_TV_UNROLL
    for (int k = 0; k < 9; k++) R1[k] = -R1[k];
  mul3(U, Wt, tmp), mul3(tmp, Vt, R2);
  if (det3(R2) < 0)
    VSG_TV_UNROLL
    for (int k = 0; k < 9; k++) R2[k] = -R2[k];
  VSG_TV_UNROLL
  for (int h = 0; h < 4; h++) {
    VSG_TV_UNROLL
    for (int k = 0; k < 9; k++) mo[h].R[k] = (h & 1) ? R2[k] : R1[k];
    VSG_TV_UNROLL
    for (int k = 0; k < 3; k++) mo[h].t[k] = h < 2 ? t[k] : -t[k];
  }
}
// ReconstructH's eight hypotheses (:583-691).  false: the singular-value gate :598
VSG_HD bool motions_h(const float *H21, const float *K, Motion *mo) {
  float invK[9], tmp[9], A[9], U[9], w[3], V[9], Vt[9];
  inverse3(K, invK);
  mul3(invK, H21, tmp), mul3(tmp, K, A);
  svd3(A, U, w, V);
  transpose3(V, Vt);
  const float s = fmul(det3(U), det3(Vt));
  const float d1 = w[0], d2 = w[1], d3 = w[2];
  if ((double)fdiv(d1, d2) < 1.00001 || (double)fdiv(d2, d3) < 1.00001) return false;
  const float d11 = fmul(d1, d1), d22 = fmul(d2, d2), d33 = fmul(d3, d3);
  const float aux1 = fsqrt(fdiv(fsub(d11, d22), fsub(d11, d33)));
  const float aux3 = fsqrt(fdiv(fsub(d22, d33), fsub(d11, d33)));
  const float root = fsqrt(fmul(fsub(d11, d22), fsub(d22, d33)));
  const float aux_stheta = fdiv(root, fmul(fadd(d1, d3), d2));
  const float ctheta = fdiv(fadd(d22, fmul(d1, d3)), fmul(fadd(d1, d3), d2));
  const float aux_sphi = fdiv(root, fmul(fsub(d1, d3), d2));
  const float cphi = fdiv(fsub(fmul(d1, d3), d22), fmul(fsub(d1, d3), d2));
  float sU[9];  // s * U * Rp * Vt: the scalar first, left to right
  VSG_TV_UNROLL
  for (int k = 0; k < 9; k++) sU[k] = fmul(s, U[k]);
  VSG_TV_UNROLL
  for (int h = 0; h < 8; h++) {
    const int i = h & 3;
    const bool second = h >= 4;  // case d' = -d2
    const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
    const float sn = (i == 0 || i == 3) ? (second ? aux_sphi : aux_stheta) : (second ? -aux_sphi : -aux_stheta);
    float Rp[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (!second)
      Rp[0] = ctheta, Rp[2] = -sn, Rp[4] = 1.0f, Rp[6] = sn, Rp[8] = ctheta;
    else
      Rp[0] = cphi, Rp[2] = sn, Rp[4] = -1.0f, Rp[6] = sn, Rp[8] = -cphi;
    mul3(sU, Rp, tmp), mul3(tmp, Vt, mo[h].R);
    const float f = second ? fadd(d1, d3) : fsub(d1, d3);
    const float tp[3] = {fmul(x1, f), fmul(0.0f, f), fmul(second ? x3 : -x3, f)};
    float t[3];
    VSG_TV_UNROLL
    for (int r = 0; r < 3; r++) t[r] = dot3(U[3 * r], U[3 * r + 1], U[3 * r + 2], tp[0], tp[1], tp[2]);
    const float tn = fsqrt(dot3(t[0], t[1], t[2], t[0], t[1], t[2]));
    VSG_TV_UNROLL
    for (int r = 0; r < 3; r++) mo[h].t[r] = fdiv(t[r], tn);
  }
  return true;
}

// ---- CheckRT (:784-898)
// what CheckRT sets up once per motion hypothesis: P1 = K [I | 0], P2 = K [R | t] (3 x 4 row-major), O2 = -R^T t
struct RtSetup {
  float P1[12], P2[12], O2[3], R[9], t[3], fx, fy, cx, cy, th2;
};
VSG_HD RtSetup rt_setup(const Motion &mo, const float *K, float sigma) {
  RtSetup c;
  VSG_TV_UNROLL
  for (int r = 0; r < 3; r++) {
    VSG_TV_UNROLL
    for (int j = 0; j < 4; j++) {
      c.P1[4 * r + j] = j < 3 ? K[3 * r + j] : 0.0f;
      const float b0 = j < 3 ? mo.R[j] : mo.t[0], b1 = j < 3 ? mo.R[3 + j] : mo.t[1], b2 = j < 3 ? mo.R[6 + j] : mo.t[2];
      c.P2[4 * r + j] = dot3(K[3 * r], K[3 * r + 1], K[3 * r + 2], b0, b1, b2);  // :812
    }
    c.O2[r] = dot3(-mo.R[r], -mo.R[3 + r], -mo.R[6 + r], mo.t[0], mo.t[1], mo.t[2]);  // :814
    c.t[r] = mo.t[r];
  }
  VSG_TV_UNROLL
  for (int k = 0; k < 9; k++) c.R[k] = mo.R[k];
  c.fx = K[0], c.fy = K[4], c.cx = K[2], c.cy = K[5];
  c.th2 = (float)dmul(4.0, (double)fmul(sigma, sigma));  // 4.0 * mSigma2 as the float parameter th2
  return c;
}
// GeometricTools::Triangulate (GeometricTools.cc:47-66) on two 3 x 4 projection matrices: A as :50-53 builds it, then the
// 4 x 4 routine of vsg_triangulate.h.  false = x3Dh(3) == 0 (deviation 3)
VSG_HD bool triangulate(float x1, float y1, float x2, float y2, const float *P1, const float *P2, float *x3D) {
  float A[16];
  VSG_TV_UNROLL
  for (int c = 0; c < 4; c++) {
    A[c] = fsub(fmul(x1, P1[8 + c]), P1[c]);
    A[4 + c] = fsub(fmul(y1, P1[8 + c]), P1[4 + c]);
    A[8 + c] = fsub(fmul(x2, P2[8 + c]), P2[c]);
    A[12 + c] = fsub(fmul(y2, P2[8 + c]), P2[4 + c]);
  }
  double v[4];
  tri_null_vector(A, v);
  const float h0 = (float)v[0], h1 = (float)v[1], h2 = (float)v[2], h3 = (float)v[3];
  if (h3 == 0) return false;
  x3D[0] = fdiv(h0, h3), x3D[1] = fdiv(h1, h3), x3D[2] = fdiv(h2, h3);
  return true;
}
// the body of CheckRT's loop for one inlier match (:823-884): p3d and cos are written when the match is counted
VSG_HD int check_rt_match(const RtSetup &c, const Match &m, float *p3d, float *cos_out) {
  float p[3];
  if (!triangulate(m.u1, m.v1, m.u2, m.v2, c.P1, c.P2, p)) return kRtSkipped;
  if (!finitef(p[0]) || !finitef(p[1]) || !finitef(p[2])) return kRtSkipped;  // :832
  const float n1[3] = {fsub(p[0], 0.0f), fsub(p[1], 0.0f), fsub(p[2], 0.0f)};  // O1 = 0
  const float dist1 = fsqrt(dot3(n1[0], n1[1], n1[2], n1[0], n1[1], n1[2]));
  const float n2[3] = {fsub(p[0], c.O2[0]), fsub(p[1], c.O2[1]), fsub(p[2], c.O2[2])};
  const float dist2 = fsqrt(dot3(n2[0], n2[1], n2[2], n2[0], n2[1], n2[2]));
  const float cosParallax = fdiv(dot3(n1[0], n1[1], n1[2], n2[0], n2[1], n2[2]), fmul(dist1, dist2));
  if (p[2] <= 0 && (double)cosParallax < 0.99998) return kRtSkipped;  // :848
  float p2[3];
  VSG_TV_UNROLL
  for (int r = 0; r < 3; r++) p2[r] = fadd(dot3(c.R[3 * r], c.R[3 * r + 1], c.R[3 * r + 2], p[0], p[1], p[2]), c.t[r]);
  if (p2[2] <= 0 && (double)cosParallax < 0.99998) return kRtSkipped;  // :854
  const float invZ1 = (float)ddiv(1.0, (double)p[2]);
  const float im1x = fadd(fmul(fmul(c.fx, p[0]), invZ1), c.cx), im1y = fadd(fmul(fmul(c.fy, p[1]), invZ1), c.cy);
  const float e1x = fsub(im1x, m.u1), e1y = fsub(im1y, m.v1);
  if (fadd(fmul(e1x, e1x), fmul(e1y, e1y)) > c.th2) return kRtSkipped;  // :865
  const float invZ2 = (float)ddiv(1.0, (double)p2[2]);
  const float im2x = fadd(fmul(fmul(c.fx, p2[0]), invZ2), c.cx), im2y = fadd(fmul(fmul(c.fy, p2[1]), invZ2), c.cy);
  const float e2x = fsub(im2x, m.u2), e2y = fsub(im2y, m.v2);
  if (fadd(fmul(e2x, e2x), fmul(e2y, e2y)) > c.th2) return kRtSkipped;  // :876
  p3d[0] = p[0], p3d[1] = p[1], p3d[2] = p[2];
  *cos_out = cosParallax;
  return (double)cosParallax < 0.99998 ? kRtTriangulated : kRtCounted;  // :883
}
// vCosParallax[min(50, size - 1)] after the sort (:889-892) as a rank count over the counted matches: cosv[i] is read
// where state[i] != kRtSkipped.  The first counted match (ascending i) whose value holds that rank.  n_good == 0 or no
// such element (a NaN cosine among them): NaN.
inline float ranked_cosine(const float *cosv, const uint8_t *state, int n, int n_good) {
  if (n_good <= 0) return __builtin_nanf("");
  const int idx = 50 < n_good - 1 ? 50 : n_good - 1;
  for (int j = 0; j < n; j++) {
    if (state[j] == kRtSkipped) continue;
    const float cj = cosv[j];
    int lo = 0, le = 0;
    for (int i = 0; i < n; i++)
      if (state[i] != kRtSkipped) lo += cosv[i] < cj ? 1 : 0, le += cosv[i] <= cj ? 1 : 0;
    if (lo <= idx && idx < le) return cj;
  }
  return __builtin_nanf("");
}

// ---- the last step: the choice among the motion hypotheses by nGood alone.  k = the chosen hypothesis (-1: none),
// reason = kOk (the parallax gate is still to come, two_view::finish) or kNoWinner.
struct Choice {
  int k, reason;
};
VSG_HD Choice choose_f(const int *nGood, int N, int minTriangulated) {  // :503-567
  const int a = nGood[0], b = nGood[1], c = nGood[2], d = nGood[3];
  const int m34 = c > d ? c : d, m234 = b > m34 ? b : m34, maxGood = a > m234 ? a : m234;
  const int n9 = (int)dmul(0.9, (double)N);
  const int nMinGood = n9 > minTriangulated ? n9 : minTriangulated;
  const double lim = dmul(0.7, (double)maxGood);
  int nsimilar = 0;
  if ((double)a > lim) nsimilar++;
  if ((double)b > lim) nsimilar++;
  if ((double)c > lim) nsimilar++;
  if ((double)d > lim) nsimilar++;
  Choice ch = {-1, kNoWinner};
  if (maxGood < nMinGood || nsimilar > 1) return ch;
  ch.reason = kOk;
  ch.k = maxGood == a ? 0 : maxGood == b ? 1 : maxGood == c ? 2 : 3;  // the if / else if chain
  return ch;
}
VSG_HD Choice choose_h(const int *nGood, int N, int minTriangulated) {  // :693-724, the parallax aside
  int bestGood = 0, secondBestGood = 0, best = -1;
  VSG_TV_UNROLL
  for (int i = 0; i < 8; i++) {
    if (nGood[i] > bestGood)
      secondBestGood = bestGood, bestGood = nGood[i], best = i;
    else if (nGood[i] > secondBestGood)
      secondBestGood = nGood[i];
  }
  Choice ch = {best, kNoWinner};
  if ((double)secondBestGood < dmul(0.75, (double)bestGood) && bestGood > minTriangulated &&
      (double)bestGood > dmul(0.9, (double)N))
    ch.reason = kOk;
  return ch;
}


// what the selection leaves behind (Reconstruct :112-128 and the decomposition of the chosen model), the same on every
// lane that asks.  best_h / best_f = first_maximum of the two score arrays; H21 / H12 / F21 = those hypotheses recomputed
// (not read where the index is -1); n_in_h / n_in_f = their inlier counts.
VSG_HD void fill_selected(Selected &S, int best_h, int best_f, float SH, float SF, const float *H21, const float *F21,
                          int n_in_h, int n_in_f, const float *K, float rh_threshold) {
  S.best_it_h = best_h, S.best_it_f = best_f, S.SH = SH, S.SF = SF;
  VSG_TV_UNROLL
  for (int k = 0; k < 9; k++) S.H21[k] = best_h >= 0 ? H21[k] : 0.0f, S.F21[k] = best_f >= 0 ? F21[k] : 0.0f;
  S.model = kModelF, S.reason = kOk, S.n_motion = 0, S.n_inliers = 0;
  VSG_TV_UNROLL
  for (int h = 0; h < 8; h++) {  // defined bytes behind n_motion
    VSG_TV_UNROLL
    for (int k = 0; k < 9; k++) S.motion[h].R[k] = 0.0f;
    VSG_TV_UNROLL
    for (int k = 0; k < 3; k++) S.motion[h].t[k] = 0.0f;
  }
  const float sum = fadd(SH, SF);
  if (sum == 0.f) {  // :112
    S.reason = kNoScore;
    return;
  }
  const float RH = fdiv(SH, sum);
  if (RH > rh_threshold) {  // :119
    S.model = kModelH, S.n_inliers = n_in_h;
    if (motions_h(S.H21, K, S.motion))
      S.n_motion = 8;
    else
      S.reason = kSingularValues;
  } else {
    S.n_inliers = n_in_f;
    motions_f(S.F21, K, S.motion);
    S.n_motion = 4;
  }
}

// ---- the host's side of a call: what is refused before anything is enqueued, the step behind the wait, and the whole
// routine on one thread (the tests' host build and the latency probe's caller-side path; the device runs vsg_two_view.hip)

// mvMatches12 (:51-63): the entries with vMatches12[i] >= 0 in ascending i as pairs {first, second}.  pairs holds 2 * n1
// ints.  The number of matches, or -1 for an entry outside [-1, n2).
inline int compact_matches(int n1, int n2, const int32_t *matches12, int32_t *pairs) {
  int N = 0;
  for (int i = 0; i < n1; i++) {
    const int m = matches12[i];
    if (m < -1 || m >= n2) return -1;
    if (m >= 0) pairs[2 * N] = i, pairs[2 * N + 1] = m, N++;
  }
  return N;
}
// every set entry lies in [0, N) and no set lists a match twice (the reference draws without replacement)
inline bool sets_ok(int N, int n_iter, const int32_t *sets) {
  for (int it = 0; it < n_iter; it++) {
    const int32_t *s = sets + 8 * (size_t)it;
    for (int j = 0; j < 8; j++) {
      if (s[j] < 0 || s[j] >= N) return false;
      for (int k = 0; k < j; k++)
        if (s[k] == s[j]) return false;
    }
  }
  return true;
}
inline bool params_ok(const float *K, const vsg_two_view_params *p, int n_iter) {
  if (!K || !p || n_iter < 1 || n_iter > kMaxIterations) return false;
  for (int k = 0; k < 9; k++)
    if (!finitef(K[k])) return false;
  return finitef(p->sigma) && p->sigma > 0;
}

// parallax = acos(vCosParallax[idx]) * 180 / CV_PI (:892): the float acos, the product in float, the quotient in double
inline float parallax_of(float cosine, int n_good) {
  if (n_good <= 0) return 0.0f;  // :895
  return (float)((double)(std::acos(cosine) * 180.0f) / 3.1415926535897932384626433832795);
}
// The step behind the wait: the parallax gate (:526 ... :559 `>`, :724 `>=`) and the result.  n_good / cosv = nGood and
// the ranked cosine of the S.n_motion hypotheses.  true = the caller's arrays are to be written.
inline bool finish(const Selected &S, const int *n_good, const float *cosv, const vsg_two_view_params &P, vsg_two_view_result *res) {
  res->ok = 0, res->reason = S.reason, res->model = S.model;
  res->SH = canonf(S.SH), res->SF = canonf(S.SF), res->best_it_h = S.best_it_h, res->best_it_f = S.best_it_f;
  for (int k = 0; k < 9; k++) res->H21[k] = canonf(S.H21[k]), res->F21[k] = canonf(S.F21[k]), res->R21[k] = 0.0f;
  for (int k = 0; k < 3; k++) res->t21[k] = 0.0f;
  for (int k = 0; k < 8; k++) res->n_good[k] = k < S.n_motion ? n_good[k] : 0;
  res->parallax = 0.0f, res->n_inliers = S.n_inliers;
  if (S.reason != kOk) return false;
  const Choice ch = S.model == kModelH ? choose_h(n_good, S.n_inliers, P.min_triangulated)
                                       : choose_f(n_good, S.n_inliers, P.min_triangulated);
  if (ch.reason != kOk) {
    res->reason = ch.reason;
    return false;
  }
  const float parallax = parallax_of(cosv[ch.k], n_good[ch.k]);
  res->parallax = canonf(parallax);
  if (S.model == kModelH ? !(parallax >= P.min_parallax) : !(parallax > P.min_parallax)) {
    res->reason = kLowParallax;
    return false;
  }
  res->ok = 1;
  for (int k = 0; k < 9; k++) res->R21[k] = canonf(S.motion[ch.k].R[k]);
  for (int k = 0; k < 3; k++) res->t21[k] = canonf(S.motion[ch.k].t[k]);
  return true;
}
// the chosen hypothesis once more, for the caller that scatters its points (finish has returned true)
inline int chosen_motion(const Selected &S, const int *n_good, int min_triangulated) {
  return (S.model == kModelH ? choose_h(n_good, S.n_inliers, min_triangulated) : choose_f(n_good, S.n_inliers, min_triangulated)).k;
}
// vbTriangulated and vP3D of the chosen hypothesis (:528-529, :727) from its per-match verdicts: both vectors are
// assigned whole (n1 entries, zero where CheckRT wrote nothing); vP3D on the F path only (x3d may then not be NULL)
inline void scatter_outputs(int n1, int N, const int32_t *pairs, const uint8_t *state, const float *pos, bool with_points,
                            uint8_t *triangulated, float *x3d) {
  for (int i = 0; i < n1; i++) triangulated[i] = 0;
  if (with_points)
    for (size_t i = 0; i < 3 * (size_t)n1; i++) x3d[i] = 0.0f;
  for (int i = 0; i < N; i++) {
    if (state[i] == kRtSkipped) continue;
    const size_t f = (size_t)pairs[2 * i];
    if (state[i] == kRtTriangulated) triangulated[f] = 1;
    if (with_points)
      for (int k = 0; k < 3; k++) x3d[3 * f + k] = canonf(pos[3 * (size_t)i + k]);
  }
}

// scratch of reconstruct_host, the caller's so that a timing loop allocates nothing
struct HostScratch {
  std::vector<int32_t> pairs;
  std::vector<Match> m;
  std::vector<float> score, cosv, pos;
  std::vector<uint8_t> in_h, in_f, state;
};
// one model's loop (:155-178 / :205-228) on the host: scores[n_iter], raw
inline void search_host(int model, int N, const Match *m, int n_iter, const int32_t *sets, const float *T1, const float *T2x,
                        float invSigmaSquare, float *scores) {
  for (int it = 0; it < n_iter; it++) {
    const int32_t *set = sets + 8 * (size_t)it;
    auto pt = [&](int j, float *p) {
      const Match &q = m[set[j]];
      p[0] = q.x1, p[1] = q.y1, p[2] = q.x2, p[3] = q.y2;
    };
    float H21[9], H12[9], F21[9], score = 0.0f, t1, t2;
    if (model == kModelH) {
      JacobiRegs<16, 9> s;
      hypothesis_h(s, pt, T1, T2x, H21, H12);
      for (int i = 0; i < N; i++) score_h(H21, H12, m[i], invSigmaSquare, &t1, &t2), score = fadd(fadd(score, t1), t2);
    } else {
      JacobiRegs<8, 9> s;
      hypothesis_f(s, pt, T1, T2x, F21);
      for (int i = 0; i < N; i++) score_f(F21, m[i], invSigmaSquare, &t1, &t2), score = fadd(fadd(score, t1), t2);
    }
    scores[it] = score;
  }
}
// TwoViewReconstruction::Reconstruct on arrays the caller holds: xy1 / xy2 = {x, y} of every undistorted keypoint of the
// two frames.  The arguments have passed compact_matches (>= 8 matches), sets_ok and params_ok.  two_threads: the two
// model searches side by side, as the reference runs them (:104-109).  Outputs as vsg_two_view_reconstruct.
inline void reconstruct_host(const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12, const float *K,
                             const vsg_two_view_params &P, int n_iter, const int32_t *sets, bool two_threads, HostScratch &W,
                             vsg_two_view_result *res, uint8_t *triangulated, float *x3d, uint8_t *inlier_h, uint8_t *inlier_f,
                             float *score_h_out, float *score_f_out) {
  W.pairs.resize(2 * (size_t)n1 + 2);
  const int N = compact_matches(n1, n2, matches12, W.pairs.data());
  const Norm nm1 = normalize(n1, [&](int i, float *x, float *y) { *x = xy1[2 * (size_t)i], *y = xy1[2 * (size_t)i + 1]; });
  const Norm nm2 = normalize(n2, [&](int i, float *x, float *y) { *x = xy2[2 * (size_t)i], *y = xy2[2 * (size_t)i + 1]; });
  float T1[9], T2[9], T2inv[9], T2t[9];
  norm_matrix(nm1, T1), norm_matrix(nm2, T2), inverse3(T2, T2inv), transpose3(T2, T2t);
  W.m.resize((size_t)N), W.score.resize(2 * (size_t)n_iter), W.in_h.assign((size_t)N, 0), W.in_f.assign((size_t)N, 0);
  for (int i = 0; i < N; i++) {
    const size_t a = (size_t)W.pairs[2 * i], b = (size_t)W.pairs[2 * i + 1];
    W.m[(size_t)i] = make_match(nm1, nm2, xy1[2 * a], xy1[2 * a + 1], xy2[2 * b], xy2[2 * b + 1]);
  }
  const Match *m = W.m.data();
  const float inv_s2 = inv_sigma_square(P.sigma);
  float *sc_h = W.score.data(), *sc_f = sc_h + n_iter;
  if (two_threads) {
    std::thread th([&] { search_host(kModelH, N, m, n_iter, sets, T1, T2inv, inv_s2, sc_h); });
    search_host(kModelF, N, m, n_iter, sets, T1, T2t, inv_s2, sc_f);
    th.join();
  } else {
    search_host(kModelH, N, m, n_iter, sets, T1, T2inv, inv_s2, sc_h);
    search_host(kModelF, N, m, n_iter, sets, T1, T2t, inv_s2, sc_f);
  }
  for (int it = 0; it < n_iter; it++) {
    if (score_h_out) score_h_out[it] = canonf(sc_h[it]);
    if (score_f_out) score_f_out[it] = canonf(sc_f[it]);
  }
  const int best_h = first_maximum(sc_h, n_iter), best_f = first_maximum(sc_f, n_iter);
  float H21[9], H12[9], F21[9], t1, t2;
  int n_in_h = 0, n_in_f = 0;
  if (best_h >= 0) {
    const int32_t *set = sets + 8 * (size_t)best_h;
    JacobiRegs<16, 9> s;
    hypothesis_h(s, [&](int j, float *p) { const Match &q = m[set[j]]; p[0] = q.x1, p[1] = q.y1, p[2] = q.x2, p[3] = q.y2; },
                 T1, T2inv, H21, H12);
    for (int i = 0; i < N; i++) n_in_h += (W.in_h[(size_t)i] = score_h(H21, H12, m[i], inv_s2, &t1, &t2) ? 1 : 0);
  }
  if (best_f >= 0) {
    const int32_t *set = sets + 8 * (size_t)best_f;
    JacobiRegs<8, 9> s;
    hypothesis_f(s, [&](int j, float *p) { const Match &q = m[set[j]]; p[0] = q.x1, p[1] = q.y1, p[2] = q.x2, p[3] = q.y2; },
                 T1, T2t, F21);
    for (int i = 0; i < N; i++) n_in_f += (W.in_f[(size_t)i] = score_f(F21, m[i], inv_s2, &t1, &t2) ? 1 : 0);
  }
  for (int i = 0; i < N; i++) {
    if (inlier_h) inlier_h[i] = W.in_h[(size_t)i];
    if (inlier_f) inlier_f[i] = W.in_f[(size_t)i];
  }
  Selected S;
  fill_selected(S, best_h, best_f, best_h >= 0 ? sc_h[best_h] : 0.0f, best_f >= 0 ? sc_f[best_f] : 0.0f, H21, F21, n_in_h,
                n_in_f, K, P.rh_threshold);
  const uint8_t *in = S.model == kModelH ? W.in_h.data() : W.in_f.data();
  int n_good[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  float cosk[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  W.state.assign(8 * (size_t)N, 0), W.cosv.assign(8 * (size_t)N, 0.0f), W.pos.assign(24 * (size_t)N, 0.0f);
  for (int h = 0; h < S.n_motion; h++) {
    const RtSetup c = rt_setup(S.motion[h], K, P.sigma);
    uint8_t *st = W.state.data() + (size_t)h * N;
    float *cv = W.cosv.data() + (size_t)h * N, *ps = W.pos.data() + 3 * (size_t)h * N;
    for (int i = 0; i < N; i++) {
      if (!in[i]) continue;  // :820
      st[i] = (uint8_t)check_rt_match(c, m[i], ps + 3 * (size_t)i, cv + i);
      n_good[h] += st[i] != kRtSkipped ? 1 : 0;
    }
    cosk[h] = ranked_cosine(cv, st, N, n_good[h]);
  }
  if (finish(S, n_good, cosk, P, res)) {
    const int k = chosen_motion(S, n_good, P.min_triangulated);
    scatter_outputs(n1, N, W.pairs.data(), W.state.data() + (size_t)k * N, W.pos.data() + 3 * (size_t)k * N, S.model == kModelF,
                    triangulated, x3d);
  }
}

}  // namespace two_view
}  // namespace vsg
