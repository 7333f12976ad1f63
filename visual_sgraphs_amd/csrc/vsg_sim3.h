// vsg_sim3.h -- Sim3Solver (Sim3Solver.cc) on point pairs in two camera frames, host and device from one source: the set-up
// of one correspondence (:103-107, :114-115), ONE RANSAC hypothesis (ComputeSim3, :307-407) and its inlier test
// (CheckInliers, :409-433), and the selection over the hypotheses' inlier counts that iterate's loop (:215-291) amounts to.
// k_sim3_points / k_sim3_hypotheses / k_sim3_select (vsg_sim3.hip) run it on the device, tests/_sim3core and the latency
// probe's caller-side path (tools/resident_points_cpu.cpp) compile it for the host.  As in vsg_triangulate.h the order is
// fixed and nothing contracts: every operation is one vsg::f* / vsg::d* call = one rounding, every comparison is written as
// the reference writes it, so that a NaN takes the reference's branch.  No libm other than sqrt.
//
// Hypothesis k depends on its three sampled correspondences alone, and the loop's stopping rule is a function of the
// counts (select below): the solver is independent work plus a selection, not a sequence.
//
// WHERE THE REFERENCE IS DOUBLE.  N11..N44 (:327-340) are doubles that HOLD float sums -- M's entries are float, so
// `M(0, 0) + M(1, 1) + M(2, 2)` is added in float and widened afterwards -- and the matrix N stores them as float again:
// N is built here in float, which is that value exactly.  `nom` and `den` (:373, :379) are Eigen reductions of nine float
// products whose order is the packet reduction of the build; here the float products are summed in double in column-major
// order.  ms12i = (float)(nom / den) with the division in double, 1.0 / ms12i (:400) likewise.
//
// TWO DEVIATIONS of arithmetic class, both measured by tests/test_sim3_reference.py:
//   1. the eigenvector of N's largest eigenvalue comes from Eigen::EigenSolver<Matrix4f>, a general (non-symmetric) solver
//      run in float, which cannot be restated bit for bit without Eigen.  Here: a cyclic Jacobi on the symmetric N in DOUBLE,
//      kSweeps sweeps over the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3); the column of the largest diagonal entry (the
//      lowest index on a tie, as maxCoeff).
//   2. the rotation goes atan2 -> 2 * ang * vec / |vec| -> Sophus::SO3f::exp in the reference.  Here the rotation matrix
//      is formed from the normalised quaternion in double and rounded to float once: no atan2, no sin / cos.  The matrix is
//      quadratic in the quaternion, so its sign (the reference's ang > pi / 2 for w < 0) changes no bit.
//      KEPT: an imaginary part whose float norm is exactly 0 makes :362 divide 0 by 0 -- R is NaN, every comparison with it
//      is false, the hypothesis has no inlier (two identical triples do that).  rotation_from_quaternion writes that case out.
#pragma once
#include <stddef.h>

#include "../../include/vsg_orb.h"
#include "vsg_frustum.h"
#include "vsg_math.h"

#if defined(__HIPCC__)
#define VSG_SIM3_UNROLL _Pragma("unroll")
#else
#define VSG_SIM3_UNROLL
#endif

namespace vsg {
namespace sim3 {

// Jacobi sweeps.  NumPy trial (this routine transcribed; the 1200 N matrices of the four scenes of tests/sim3_scenes.py,
// 1189 of them with the two largest eigenvalues >= 1e-2 apart, relative): against numpy.linalg.eigh the largest component
// error of the unit eigenvector of those 1189 was 8.3e-1 / 1.6e-1 / 2.0e-3 / 2.8e-8 / 2.0e-14 after 1 .. 5 sweeps and
// stayed 2.0e-14 from there on (the conditioning: 1e-16 over the gap); the 11 near-collinear triples, their error scaled
// by the gap, were final (2.8e-16) after 4.  One more than the 5 it took.
enum { kSweeps = 6 };
enum { kMaxHypotheses = 1024 };

// what the solver keeps of one correspondence (mvX3Dc1/2, mvP1im1, mvP2im2, mvnMaxError1/2 as the comparison sees them)
struct Point {
  float X1[3], X2[3], p1[2], p2[2], max_err1, max_err2;
};
struct Camera {
  float fx, fy, cx, cy;
};
// mR12i (row-major), mt12i, ms12i, mT12i, mT21i (row-major)
struct Hypothesis {
  float R12[9], t12[3], s12, T12[16], T21[16];
};
struct Selection {
  int best, converged, iterations;  // k, bConverge, mnIterations
};

VSG_HD float canonf(float v) { return v != v ? __builtin_nanf("") : v; }
VSG_HD Camera camera_of(const vsg_frame_pose &p) { return Camera{p.fx, p.fy, p.cx, p.cy}; }

// Rcw * Xw + tcw (:104, :107)
VSG_HD void camera_point(const vsg_frame_pose &c, const float *Xw, float *Xc) {
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++)
    Xc[r] = fadd(dot3(c.Rcw[3 * r], c.Rcw[3 * r + 1], c.Rcw[3 * r + 2], Xw[0], Xw[1], Xw[2]), c.tcw[r]);
}
// Pinhole::project (Pinhole.cpp:46-53)
VSG_HD void project(const Camera &c, const float *X, float *p) {
  p[0] = fadd(fdiv(fmul(c.fx, X[0]), X[2]), c.cx);
  p[1] = fadd(fdiv(fmul(c.fy, X[1]), X[2]), c.cy);
}
// one correspondence: both world positions through their keyframes' poses -- kf2's also for a point matched through
// another keyframe (:107) -- and their images
VSG_HD Point make_point(const vsg_frame_pose &kf1, const vsg_frame_pose &kf2, const float *Xw1, const float *Xw2, float max_err1,
                        float max_err2) {
  Point p;
  camera_point(kf1, Xw1, p.X1), camera_point(kf2, Xw2, p.X2);
  project(camera_of(kf1), p.X1, p.p1), project(camera_of(kf2), p.X2, p.p2);
  p.max_err1 = max_err1, p.max_err2 = max_err2;
  return p;
}

// ComputeCentroid (:299-305): P[3 c + r] = row r of column c.  The sum of a row is Eigen's unrolled reduction of three,
// a0 + (a1 + a2); C / P.cols() divides by 3.
VSG_HD void centroid(const float *P, float *Pr, float *C) {
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++) C[r] = fdiv(fadd(P[r], fadd(P[3 + r], P[6 + r])), 3.0f);
  VSG_SIM3_UNROLL
  for (int c = 0; c < 3; c++)
    VSG_SIM3_UNROLL
    for (int r = 0; r < 3; r++) Pr[3 * c + r] = fsub(P[3 * c + r], C[r]);
}

// Eigenvector of the largest eigenvalue of the symmetric 4 x 4 N (row-major float), in double, not normalised further
// than the rotations leave it (unit up to rounding).  Loops are compile-time bounded and every index is a constant after
// unrolling, so A and V stay in registers.  A rotation of an exactly zero off-diagonal entry is skipped.
VSG_HD void largest_eigenvector(const float *N, double *q) {
  double A[4][4], V[4][4];
  VSG_SIM3_UNROLL
  for (int r = 0; r < 4; r++)
    VSG_SIM3_UNROLL
    for (int c = 0; c < 4; c++) A[r][c] = (double)N[4 * r + c], V[r][c] = r == c ? 1.0 : 0.0;
  VSG_SIM3_UNROLL
  for (int sweep = 0; sweep < kSweeps; sweep++) {
    VSG_SIM3_UNROLL
    for (int p = 0; p < 3; p++) {
      VSG_SIM3_UNROLL
      for (int r = p + 1; r < 4; r++) {
        const double apq = A[p][r];
        if (apq == 0.0) continue;
        const double theta = ddiv(dsub(A[r][r], A[p][p]), dmul(2.0, apq));
        const double at = theta < 0.0 ? -theta : theta;
        const double ta = ddiv(1.0, dadd(at, dsqrt(dadd(dmul(theta, theta), 1.0))));
        const double t = theta < 0.0 ? -ta : ta;
        const double c = ddiv(1.0, dsqrt(dadd(dmul(t, t), 1.0))), s = dmul(t, c);
        A[p][p] = dsub(A[p][p], dmul(t, apq)), A[r][r] = dadd(A[r][r], dmul(t, apq));
        A[p][r] = 0.0, A[r][p] = 0.0;
        VSG_SIM3_UNROLL
        for (int k = 0; k < 4; k++) {
          if (k != p && k != r) {
            const double akp = A[k][p], akq = A[k][r];
            const double np = dsub(dmul(c, akp), dmul(s, akq)), nq = dadd(dmul(s, akp), dmul(c, akq));
            A[k][p] = np, A[p][k] = np, A[k][r] = nq, A[r][k] = nq;
          }
          const double vp = V[k][p], vq = V[k][r];
          V[k][p] = dsub(dmul(c, vp), dmul(s, vq)), V[k][r] = dadd(dmul(s, vp), dmul(c, vq));
        }
      }
    }
  }
  double best = A[0][0];
  VSG_SIM3_UNROLL
  for (int k = 0; k < 4; k++) q[k] = V[k][0];
  VSG_SIM3_UNROLL
  for (int c = 1; c < 4; c++) {
    if (A[c][c] > best) {  // maxCoeff: the first of equal maxima
      best = A[c][c];
      VSG_SIM3_UNROLL
      for (int k = 0; k < 4; k++) q[k] = V[k][c];
    }
  }
}

// mR12i of the quaternion q = (w, x, y, z) (:357-363).  The reference's vec is the float eigenvector's imaginary part
// and vec.norm() its float norm: exactly 0 (underflow included) gives 0 / 0 at :362 and a NaN rotation.
VSG_HD void rotation_from_quaternion(const double *q, float *R) {
  const float vx = (float)q[1], vy = (float)q[2], vz = (float)q[3];
  if (fsqrt(fadd(fmul(vx, vx), fadd(fmul(vy, vy), fmul(vz, vz)))) == 0) {
    VSG_SIM3_UNROLL
    for (int k = 0; k < 9; k++) R[k] = __builtin_nanf("");
    return;
  }
  const double n = dsqrt(dadd(dadd(dmul(q[0], q[0]), dmul(q[1], q[1])), dadd(dmul(q[2], q[2]), dmul(q[3], q[3]))));
  const double w = ddiv(q[0], n), x = ddiv(q[1], n), y = ddiv(q[2], n), z = ddiv(q[3], n);
  const double xx = dmul(x, x), yy = dmul(y, y), zz = dmul(z, z), xy = dmul(x, y), xz = dmul(x, z), yz = dmul(y, z);
  const double wx = dmul(w, x), wy = dmul(w, y), wz = dmul(w, z);
  R[0] = (float)dsub(1.0, dmul(2.0, dadd(yy, zz))), R[1] = (float)dmul(2.0, dsub(xy, wz)), R[2] = (float)dmul(2.0, dadd(xz, wy));
  R[3] = (float)dmul(2.0, dadd(xy, wz)), R[4] = (float)dsub(1.0, dmul(2.0, dadd(xx, zz))), R[5] = (float)dmul(2.0, dsub(yz, wx));
  R[6] = (float)dmul(2.0, dsub(xz, wy)), R[7] = (float)dmul(2.0, dadd(yz, wx)), R[8] = (float)dsub(1.0, dmul(2.0, dadd(xx, yy)));
}

// N of :327-345 from M (row-major), row-major
VSG_HD void horn_matrix(const float *M, float *N) {
  const float m00 = M[0], m01 = M[1], m02 = M[2], m10 = M[3], m11 = M[4], m12 = M[5], m20 = M[6], m21 = M[7], m22 = M[8];
  const float N11 = fadd(fadd(m00, m11), m22), N12 = fsub(m12, m21), N13 = fsub(m20, m02), N14 = fsub(m01, m10);
  const float N22 = fsub(fsub(m00, m11), m22), N23 = fadd(m01, m10), N24 = fadd(m20, m02);
  const float N33 = fsub(fadd(-m00, m11), m22), N34 = fadd(m12, m21), N44 = fadd(fsub(-m00, m11), m22);
  N[0] = N11, N[1] = N12, N[2] = N13, N[3] = N14;
  N[4] = N12, N[5] = N22, N[6] = N23, N[7] = N24;
  N[8] = N13, N[9] = N23, N[10] = N33, N[11] = N34;
  N[12] = N14, N[13] = N24, N[14] = N34, N[15] = N44;
}

// ComputeSim3 (:307-407).  P1 / P2: the three sampled X3Dc1 / X3Dc2 as columns 0..2 (P[3 c + r]).  N_out (may be
// nullptr): the float N, for the tests.
VSG_HD Hypothesis compute_sim3(const float *P1, const float *P2, bool fix_scale, float *N_out) {
  Hypothesis h;
  float Pr1[9], Pr2[9], O1[3], O2[3];
  centroid(P1, Pr1, O1), centroid(P2, Pr2, O2);  // :319-320
  float M[9];                                    // :324: M = Pr2 * Pr1^T, the sum over the columns in order
  VSG_SIM3_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_SIM3_UNROLL
    for (int j = 0; j < 3; j++) M[3 * i + j] = dot3(Pr2[i], Pr2[3 + i], Pr2[6 + i], Pr1[j], Pr1[3 + j], Pr1[6 + j]);
  float N[16];
  horn_matrix(M, N);
  if (N_out)
    for (int k = 0; k < 16; k++) N_out[k] = N[k];
  double q[4];
  largest_eigenvector(N, q);          // :348-355 (deviation 1)
  rotation_from_quaternion(q, h.R12);  // :357-363 (deviation 2)
  const float *R = h.R12;
  float P3[9];  // :366: P3 = mR12i * Pr2
  VSG_SIM3_UNROLL
  for (int c = 0; c < 3; c++)
    VSG_SIM3_UNROLL
    for (int r = 0; r < 3; r++) P3[3 * c + r] = dot3(R[3 * r], R[3 * r + 1], R[3 * r + 2], Pr2[3 * c], Pr2[3 * c + 1], Pr2[3 * c + 2]);
  if (!fix_scale) {  // :370-382
    double nom = 0.0, den = 0.0;
    VSG_SIM3_UNROLL
    for (int k = 0; k < 9; k++) nom = dadd(nom, (double)fmul(Pr1[k], P3[k])), den = dadd(den, (double)fmul(P3[k], P3[k]));
    h.s12 = (float)ddiv(nom, den);
  } else {
    h.s12 = 1.0f;
  }
  float sR[9];  // :394
  VSG_SIM3_UNROLL
  for (int k = 0; k < 9; k++) sR[k] = fmul(h.s12, R[k]);
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++) h.t12[r] = fsub(O1[r], dot3(sR[3 * r], sR[3 * r + 1], sR[3 * r + 2], O2[0], O2[1], O2[2]));  // :387
  const float inv = (float)ddiv(1.0, (double)h.s12);  // :400: the double quotient as the float matrix's scalar
  float sRinv[9];
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++)
    VSG_SIM3_UNROLL
    for (int c = 0; c < 3; c++) sRinv[3 * r + c] = fmul(inv, R[3 * c + r]);
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++) {
    const float tinv = -dot3(sRinv[3 * r], sRinv[3 * r + 1], sRinv[3 * r + 2], h.t12[0], h.t12[1], h.t12[2]);  // :405
    VSG_SIM3_UNROLL
    for (int c = 0; c < 3; c++) h.T12[4 * r + c] = sR[3 * r + c], h.T21[4 * r + c] = sRinv[3 * r + c];
    h.T12[4 * r + 3] = h.t12[r], h.T21[4 * r + 3] = tinv;
  }
  VSG_SIM3_UNROLL
  for (int c = 0; c < 4; c++) h.T12[12 + c] = h.T21[12 + c] = c == 3 ? 1.0f : 0.0f;
  return h;
}

// the hypothesis of three correspondences (:245-258): sample j fills column j
VSG_HD Hypothesis hypothesis_of(const Point &a, const Point &b, const Point &c, bool fix_scale) {
  float P1[9], P2[9];
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++) {
    P1[r] = a.X1[r], P1[3 + r] = b.X1[r], P1[6 + r] = c.X1[r];
    P2[r] = a.X2[r], P2[3 + r] = b.X2[r], P2[6 + r] = c.X2[r];
  }
  return compute_sim3(P1, P2, fix_scale, nullptr);
}

// Project (:455-469) of one point through T (row-major 4 x 4)
VSG_HD void project_through(const float *T, const Camera &cam, const float *X, float *p) {
  float Xc[3];
  VSG_SIM3_UNROLL
  for (int r = 0; r < 3; r++) Xc[r] = fadd(dot3(T[4 * r], T[4 * r + 1], T[4 * r + 2], X[0], X[1], X[2]), T[4 * r + 3]);
  project(cam, Xc, p);
}
// CheckInliers' test of one correspondence (:412-425); err (may be nullptr): {err1, err2}
VSG_HD bool is_inlier(const Hypothesis &h, const Camera &cam1, const Camera &cam2, const Point &p, float *err) {
  float p2im1[2], p1im2[2];
  project_through(h.T12, cam1, p.X2, p2im1);
  project_through(h.T21, cam2, p.X1, p1im2);
  const float d10 = fsub(p.p1[0], p2im1[0]), d11 = fsub(p.p1[1], p2im1[1]);
  const float d20 = fsub(p1im2[0], p.p2[0]), d21 = fsub(p1im2[1], p.p2[1]);
  const float err1 = fadd(fmul(d10, d10), fmul(d11, d11)), err2 = fadd(fmul(d20, d20), fmul(d21, d21));
  if (err) err[0] = err1, err[1] = err2;
  return err1 < p.max_err1 && err2 < p.max_err2;
}

// What iterate's loop (:237-285), called until bConverge || bNoMore, leaves behind, from the inlier counts c[0 .. n_hyp)
// of the hypotheses in order.  A hypothesis is kept when c >= the best so far (0 at the start: hypothesis 0 is always kept,
// a tie goes to the later one) and the loop returns at the first kept one with c > min_inliers -- which is the first one
// above min_inliers at all, because the best so far cannot exceed it while the loop runs.  Otherwise every hypothesis is
// walked and the members hold the LAST one that reaches the maximum.
VSG_HD Selection select(const int32_t *c, int n_hyp, int min_inliers) {
  Selection s = {0, 0, n_hyp};
  int best = 0;
  for (int k = 0; k < n_hyp; k++) {
    const int ck = c[k];
    if (ck >= best) {
      best = ck, s.best = k;
      if (ck > min_inliers) {
        s.converged = 1, s.iterations = k + 1;
        return s;
      }
    }
  }
  return s;
}

// the result of a call as vsg_sim3_result holds it, NaNs canonicalised
VSG_HD void fill_result(const Hypothesis &h, const Selection &s, int n_inliers, vsg_sim3_result *res) {
  for (int k = 0; k < 9; k++) res->R12[k] = canonf(h.R12[k]);
  for (int k = 0; k < 3; k++) res->t12[k] = canonf(h.t12[k]);
  res->s12 = canonf(h.s12);
  for (int k = 0; k < 16; k++) res->T12[k] = canonf(h.T12[k]);
  res->converged = s.converged, res->no_more = s.converged ? 0 : 1, res->n_inliers = n_inliers, res->best_hypothesis = s.best;
  res->iterations = s.iterations;
}
// N < mRansacMinInliers (:222-226): bNoMore, the identity, nothing computed
inline void fill_no_more(vsg_sim3_result *res) {
  for (int k = 0; k < 9; k++) res->R12[k] = k % 4 == 0 ? 1.0f : 0.0f;
  for (int k = 0; k < 3; k++) res->t12[k] = 0.0f;
  res->s12 = 1.0f;
  for (int k = 0; k < 16; k++) res->T12[k] = k % 5 == 0 ? 1.0f : 0.0f;
  res->converged = 0, res->no_more = 1, res->n_inliers = 0, res->best_hypothesis = -1, res->iterations = 0;
}

// ---- the host's side of a call: what is refused before anything is enqueued as far as it needs no store, and the whole
// solve on one thread (the tests' host build and the latency probe's caller-side path; the device runs vsg_sim3.hip)

inline bool args_ok(int n, const int32_t *slots1, const int32_t *slots2, const float *max_err1, const float *max_err2,
                    int min_inliers, int n_hyp, const int32_t *samples, const uint8_t *inlier) {
  if (n < 0 || min_inliers < 0 || n_hyp < 1 || n_hyp > kMaxHypotheses || !samples) return false;
  if (n > 0 && (!slots1 || !slots2 || !max_err1 || !max_err2 || !inlier)) return false;
  if (n < min_inliers) return true;  // nothing is computed: the samples are not read
  if (n < 3) return false;
  for (int k = 0; k < n_hyp; k++) {
    const int a = samples[3 * k], b = samples[3 * k + 1], c = samples[3 * k + 2];
    if (a < 0 || a >= n || b < 0 || b >= n || c < 0 || c >= n || a == b || a == c || b == c) return false;
  }
  return true;
}
inline bool slots_ok(int n, const int32_t *slots, int capacity) {
  for (int i = 0; i < n; i++)
    if (slots[i] < 0 || slots[i] >= capacity) return false;
  return true;
}

// vsg_mappoints_sim3_ransac on positions the caller holds: Xw1 / Xw2 = 3 n floats, GetWorldPos of both point sets.
// early_exit: stop at the first hypothesis above min_inliers as the reference's loop does (hyp_inliers / hyp_T12 are then
// written up to that hypothesis only); without it every hypothesis is computed, as on the device.  The outputs are the same
// either way.  The arguments have passed args_ok.
inline void ransac_host(int n, const float *Xw1, const float *Xw2, const float *max_err1, const float *max_err2,
                        const vsg_frame_pose &kf1, const vsg_frame_pose &kf2, bool fix_scale, int min_inliers, int n_hyp,
                        const int32_t *samples, bool early_exit, Point *pts /* n, scratch */, int32_t *counts /* n_hyp, scratch */,
                        uint8_t *inlier, vsg_sim3_result *res, int32_t *hyp_inliers, float *hyp_T12) {
  for (int i = 0; i < n; i++) inlier[i] = 0;
  if (n < min_inliers) {
    fill_no_more(res);
    return;
  }
  const Camera cam1 = camera_of(kf1), cam2 = camera_of(kf2);
  for (int i = 0; i < n; i++) pts[i] = make_point(kf1, kf2, Xw1 + 3 * (size_t)i, Xw2 + 3 * (size_t)i, max_err1[i], max_err2[i]);
  int computed = 0;
  for (int k = 0; k < n_hyp; k++) {
    const Hypothesis h = hypothesis_of(pts[samples[3 * k]], pts[samples[3 * k + 1]], pts[samples[3 * k + 2]], fix_scale);
    int c = 0;
    for (int i = 0; i < n; i++) c += is_inlier(h, cam1, cam2, pts[i], nullptr) ? 1 : 0;
    counts[k] = c, computed = k + 1;
    if (hyp_inliers) hyp_inliers[k] = c;
    if (hyp_T12)
      for (int j = 0; j < 16; j++) hyp_T12[16 * (size_t)k + j] = canonf(h.T12[j]);
    if (early_exit && c > min_inliers) break;
  }
  const Selection s = select(counts, computed, min_inliers);
  const Hypothesis h = hypothesis_of(pts[samples[3 * s.best]], pts[samples[3 * s.best + 1]], pts[samples[3 * s.best + 2]], fix_scale);
  for (int i = 0; i < n; i++) inlier[i] = is_inlier(h, cam1, cam2, pts[i], nullptr) ? 1 : 0;
  fill_result(h, s, counts[s.best], res);
}

}  // namespace sim3
}  // namespace vsg
