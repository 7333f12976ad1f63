// vsg_pose_opt.h -- Optimizer::PoseOptimization (Optimizer.cc:1063-1452, the !mpCamera2 branches) for ONE frame, host
// and device from one source: k_pose_optimize (vsg_pose.hip) runs it as one persistent workgroup, tests/_posecore and the
// latency probe's caller-side loop (tools/resident_points_cpu.cpp) compile it for the host.
//
// Everything is double, as g2o has it.  What is restated, and from where:
//   * the two edges: EdgeSE3ProjectXYZOnlyPose (OptimizableTypes.h:45, OptimizableTypes.cpp:47-62) through
//     Pinhole::project / projectJac (Pinhole.cpp:37-44, :78-89), and EdgeStereoSE3ProjectXYZOnlyPose
//     (types_six_dof_expmap.h:215-245, .cpp:365-437; its cam_project rounds 1 / z to FLOAT, its Jacobian does not);
//   * RobustKernelHuber::robustify (robust_kernel_impl.cpp:78) and BaseUnaryEdge::constructQuadraticForm
//     (base_unary_edge.hpp:43-72): b -= rho1 J^T Omega e, H += J^T (rho1 Omega) J;
//   * the dense solve of linear_solver_dense.h as an LDL^T without pivoting (Eigen's pivots);
//   * SE3Quat::exp and the left-multiplying update with its normalisation (se3quat.h:112-119, :239-269, :292-299);
//   * OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale (optimization_algorithm_levenberg.cpp:
//     61-194) under SparseOptimizer::optimize (sparse_optimizer.cpp:399-), and the round loop with its classification.
//
// Both builds use -ffp-contract=off, so every operator below is one IEEE 754 rounding on either side.  Functions whose
// rounding IEEE 754 does not define are written out here (sincos_pose); pow(x, 3) is x * x * x.  Division and sqrt are
// the language's: both are correctly rounded in the host build and, for f64, in hipcc's gfx950 lowering as far as the
// bit-for-bit GPU test can tell.
//
// SUMS OVER EDGES are taken in one fixed tree that the host replays (Team below): thread tid of kThreads sums its edges
// tid, tid + kThreads, ... serially, a butterfly over the 64 lanes of each wave follows (xor 1, 2, 4, 8, 16, 32), then
// the waves' sums are added serially, wave 0 first.  IEEE addition commutes, so every lane of the butterfly holds the
// same bits.  A NaN's payload is the one thing a sum may carry differently on the two sides: outputs are canonicalised.
//
// Every loop has a compile-time bound (4 rounds, 10 iterations, 10 trials): no input can keep the kernel running.
#pragma once
#include <stdint.h>

#include <vector>

#include "vsg_math.h"

namespace vsg {
namespace pose {

enum { kThreads = 256, kWave = 64, kWaves = kThreads / kWave, kAcc = 28, kRounds = 4, kIters = 10, kTrials = 10 };
enum { kStereo = 1, kOutlier = 2, kRemoved = 4, kGone = 8 };  // Edge flags; kGone: removeEdge has run for it
enum { kModeAll = 0, kModeHold = 1, kModeResume = 2 };

struct Cam {
  double fx, fy, cx, cy, bf;  // the Frame's floats, widened
};
struct Est {
  double q[4], t[3];  // unit quaternion x y z w, translation
};
// one edge: 64 bytes.  chi2 = the edge's chi2() as the last computeError left it (the STALE-error rule lives here)
struct Edge {
  double X[3], obs[3], w, chi2;
};
// what outlives a held call, at the head of the frame's pose buffer
struct Ctl {
  Cam cam;
  Est input, est;
  int32_t n_edges, robust, edges_left, n_bad, rounds_run, held;
};

VSG_HD double canon(double v) { return v != v ? __builtin_nan("") : v; }
VSG_HD float canonf(float v) { return v != v ? __builtin_nanf("") : v; }

// ---- sin and cos of SE3Quat::exp's theta, one source for both sides.  Cody-Waite reduction by pi/2 in three parts
// (two rounds, 118 bits of pi/2) and the fdlibm kernels' polynomials; within 2 ulp of libm on [0, pi] (the CPU test
// measures it).  theta is a norm, so >= 0; beyond 1e5 or NaN both results are NaN (the trial is then rejected).
VSG_HD void sincos_pose(double x, double *s, double *c) {
  if (!(x <= 1.0e5)) {
    *s = *c = __builtin_nan("");
    return;
  }
  const double invpio2 = 6.36619772367581382433e-01, pio2_1 = 1.57079632673412561417e+00,
               pio2_1t = 6.07710050650619224932e-11, pio2_2 = 6.07710050630396597660e-11,
               pio2_2t = 2.02226624879595063154e-21;
  const double fn = __builtin_floor(x * invpio2 + 0.5);
  double r = x - fn * pio2_1, w = fn * pio2_1t;
  const double t = r;
  w = fn * pio2_2;
  r = t - w;
  w = fn * pio2_2t - ((t - r) - w);
  const double y0 = r - w, y1 = (r - y0) - w;
  const int n = (int)fn & 3;
  const double z = y0 * y0, zz = z * z;
  // __kernel_sin(y0, y1, 1)
  const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
               S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
  const double rs = S2 + z * (S3 + z * S4) + z * zz * (S5 + z * S6), v = z * y0;
  const double ks = y0 - ((z * (0.5 * y1 - v * rs) - y1) - v * S1);
  // __kernel_cos(y0, y1)
  const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
               C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
  const double rc = z * (C1 + z * (C2 + z * C3)) + (zz * zz) * (C4 + z * (C5 + z * C6));
  const double hz = 0.5 * z, wc = 1.0 - hz;
  const double kc = wc + (((1.0 - wc) - hz) + (z * rc - y0 * y1));
  *s = n == 0 ? ks : n == 1 ? kc : n == 2 ? -ks : -kc;
  *c = n == 0 ? kc : n == 1 ? -ks : n == 2 ? -kc : ks;
}

// ---- quaternions as Eigen has them (coefficients x y z w)
VSG_HD void quat_rotate(const double *q, const double *v, double *o) {  // Quaternion::_transformVector
  const double ux = 2.0 * (q[1] * v[2] - q[2] * v[1]), uy = 2.0 * (q[2] * v[0] - q[0] * v[2]),
               uz = 2.0 * (q[0] * v[1] - q[1] * v[0]);
  o[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
  o[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
  o[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}
VSG_HD void quat_mul(const double *a, const double *b, double *o) {
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  o[0] = x, o[1] = y, o[2] = z, o[3] = w;
}
VSG_HD void quat_normalize(double *q) {  // SE3Quat::normalizeRotation
  if (q[3] < 0) q[0] *= -1, q[1] *= -1, q[2] *= -1, q[3] *= -1;
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  q[0] /= n, q[1] /= n, q[2] /= n, q[3] /= n;
}
VSG_HD void quat_from_matrix(const double m[3][3], double *q) {  // Eigen's quaternionbase_assign_impl<Matrix3d>
  double t = m[0][0] + m[1][1] + m[2][2];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t, q[1] = (m[0][2] - m[2][0]) * t, q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0);
    q[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (m[k][j] - m[j][k]) * t;
    q[j] = (m[j][i] + m[i][j]) * t;
    q[k] = (m[k][i] + m[i][k]) * t;
  }
}

// vSE3->setEstimate(SE3Quat(Tcw.unit_quaternion().cast<double>(), Tcw.translation().cast<double>())) (:1082, :1264)
VSG_HD Est est_from_pose(const float *q, const float *t) {
  Est e;
  for (int i = 0; i < 4; i++) e.q[i] = (double)q[i];
  for (int i = 0; i < 3; i++) e.t[i] = (double)t[i];
  quat_normalize(e.q);
  return e;
}

// setEstimate(SE3Quat::exp(update) * estimate()) (VertexSE3Expmap::oplusImpl): update = [omega, upsilon]
VSG_HD Est est_oplus(const Est &cur, const double *u) {
  const double th = sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  const double O[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
  double O2[3][3], R[3][3], V[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
  if (th < 0.00001) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) R[i][j] = V[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
  } else {
    double s, c;
    sincos_pose(th, &s, &c);
    const double a = s / th, b = (1.0 - c) / (th * th), d = (th - s) / (th * th * th);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        const double I = i == j ? 1.0 : 0.0;
        R[i][j] = (I + a * O[i][j]) + b * O2[i][j];
        V[i][j] = (I + b * O[i][j]) + d * O2[i][j];
      }
  }
  Est e;
  quat_from_matrix(R, e.q);
  for (int i = 0; i < 3; i++) e.t[i] = (V[i][0] * u[3] + V[i][1] * u[4]) + V[i][2] * u[5];
  quat_normalize(e.q);  // SE3Quat(const Quaterniond &, const Vector3d &)
  double rt[3], q2[4];
  quat_rotate(e.q, cur.t, rt);
  for (int i = 0; i < 3; i++) e.t[i] = e.t[i] + rt[i];
  quat_mul(e.q, cur.q, q2);
  for (int i = 0; i < 4; i++) e.q[i] = q2[i];
  quat_normalize(e.q);
  return e;
}

// ---- the edges.  computeError + chi2(): information = invSigma2 * I, multiplied out with its zeros as Eigen does
// (0 * inf is NaN there too).  Returns chi2; e[] = the error (2 or 3 rows).
VSG_HD double edge_error(const Cam &K, const Est &T, const Edge &E, bool stereo, double *e, double *Xc) {
  double r[3];
  quat_rotate(T.q, E.X, r);
  Xc[0] = r[0] + T.t[0], Xc[1] = r[1] + T.t[1], Xc[2] = r[2] + T.t[2];
  const double w = E.w;
  if (!stereo) {
    e[0] = E.obs[0] - (K.fx * Xc[0] / Xc[2] + K.cx);
    e[1] = E.obs[1] - (K.fy * Xc[1] / Xc[2] + K.cy);
    e[2] = 0.0;
    return e[0] * (w * e[0] + 0.0 * e[1]) + e[1] * (0.0 * e[0] + w * e[1]);
  }
  const double invz = (double)(float)(1.0 / Xc[2]);  // const float invz = 1.0f / trans_xyz[2]
  const double u = Xc[0] * invz * K.fx + K.cx;
  e[0] = E.obs[0] - u;
  e[1] = E.obs[1] - (Xc[1] * invz * K.fy + K.cy);
  e[2] = E.obs[2] - (u - K.bf * invz);
  return (e[0] * ((w * e[0] + 0.0 * e[1]) + 0.0 * e[2]) + e[1] * ((0.0 * e[0] + w * e[1]) + 0.0 * e[2])) +
         e[2] * ((0.0 * e[0] + 0.0 * e[1]) + w * e[2]);
}

// linearizeOplus: J[row][6], rows = 2 (mono) or 3 (stereo)
VSG_HD void edge_jacobian(const Cam &K, const double *Xc, bool stereo, double J[3][6]) {
  const double x = Xc[0], y = Xc[1], z = Xc[2];
  if (!stereo) {
    // -pCamera->projectJac(xyz_trans) * SE3deriv, the 2x3 by 3x6 product summed in k order with its zero terms
    const double P[2][3] = {{K.fx / z, 0.0, -K.fx * x / (z * z)}, {0.0, K.fy / z, -K.fy * y / (z * z)}};
    const double D[3][6] = {{0.0, z, -y, 1.0, 0.0, 0.0}, {-z, 0.0, x, 0.0, 1.0, 0.0}, {y, -x, 0.0, 0.0, 0.0, 1.0}};
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 6; j++) J[i][j] = (-P[i][0] * D[0][j] + -P[i][1] * D[1][j]) + -P[i][2] * D[2][j];
    for (int j = 0; j < 6; j++) J[2][j] = 0.0;
    return;
  }
  const double invz = 1.0 / z, invz_2 = invz * invz;
  J[0][0] = x * y * invz_2 * K.fx;
  J[0][1] = -(1 + (x * x * invz_2)) * K.fx;
  J[0][2] = y * invz * K.fx;
  J[0][3] = -invz * K.fx;
  J[0][4] = 0;
  J[0][5] = x * invz_2 * K.fx;
  J[1][0] = (1 + y * y * invz_2) * K.fy;
  J[1][1] = -x * y * invz_2 * K.fy;
  J[1][2] = -x * invz * K.fy;
  J[1][3] = 0;
  J[1][4] = -invz * K.fy;
  J[1][5] = y * invz_2 * K.fy;
  J[2][0] = J[0][0] - K.bf * y * invz_2;
  J[2][1] = J[0][1] + K.bf * x * invz_2;
  J[2][2] = J[0][2];
  J[2][3] = J[0][3];
  J[2][4] = 0;
  J[2][5] = J[0][5] - K.bf * invz_2;
}

// deltaMono = sqrt(5.991), deltaStereo = sqrt(7.815) as FLOATs (:1103-1104), the values of glibc's correctly rounded
// sqrt narrowed to float; RobustKernelHuber::setDelta squares the widened float
VSG_HD double huber_delta(bool stereo) { return stereo ? (double)2.7955322265625f : (double)2.44765186309814453125f; }

// robustify: rho0 (the cost) and rho1 (the weight)
VSG_HD void huber(double e, double delta, double *rho0, double *rho1) {
  const double dsqr = delta * delta;
  if (e <= dsqr) {
    *rho0 = e, *rho1 = 1.0;
  } else {
    const double sqrte = sqrt(e);
    *rho0 = 2 * sqrte * delta - dsqr;
    *rho1 = delta / sqrte;
  }
}

// One thread's part of an evaluation: its edges tid, tid + kThreads, ... in that order.  An edge that is an outlier
// (level 1) or removed is not active and contributes nothing.  build: acc[0] = activeRobustChi2's part, acc[1..6] the
// part of -b, acc[7..27] the upper triangle of H row by row; else acc[0] alone.  Both store the edge's chi2.
VSG_HD void thread_partial(const Cam &K, const Est &T, Edge *edges, const uint8_t *flags, int n_edges, int tid, bool robust,
                           bool build, double *acc) {
  for (int k = 0; k < (build ? (int)kAcc : 1); k++) acc[k] = 0.0;
  for (int i = tid; i < n_edges; i += kThreads) {
    const uint8_t f = flags[i];
    if (f & (kOutlier | kRemoved)) continue;
    const bool stereo = (f & kStereo) != 0;
    const Edge E = edges[i];
    double e[3], Xc[3];
    const double chi2 = edge_error(K, T, E, stereo, e, Xc);
    edges[i].chi2 = chi2;
    double rho0 = chi2, rho1 = 1.0;
    if (robust) huber(chi2, huber_delta(stereo), &rho0, &rho1);
    acc[0] = acc[0] + rho0;
    if (!build) continue;
    double J[3][6];
    edge_jacobian(K, Xc, stereo, J);
    const int rows = stereo ? 3 : 2;
    const double wo = rho1 * E.w;
    int h = 7;
    for (int a = 0; a < 6; a++) {
      double b = 0.0;
      for (int r = 0; r < rows; r++) b = b + ((rho1 * J[r][a]) * E.w) * e[r];
      acc[1 + a] = acc[1 + a] + b;
      for (int c = a; c < 6; c++, h++) {
        double s = 0.0;
        for (int r = 0; r < rows; r++) s = s + (J[r][a] * wo) * J[r][c];
        acc[h] = acc[h] + s;
      }
    }
  }
}

// (H + lambda I) x = b by LDL^T without pivoting.  false = a pivot <= 0 (not positive: the caller's tempChi becomes
// DBL_MAX); a NaN pivot passes, as it does Eigen's sign test, and x comes out NaN.
VSG_HD bool solve6(const double *acc, double lambda, double *x) {
  double A[6][6], L[6][6], D[6], y[6];
  int h = 7;
  for (int a = 0; a < 6; a++)
    for (int c = a; c < 6; c++, h++) A[a][c] = A[c][a] = acc[h];
  for (int a = 0; a < 6; a++) A[a][a] = A[a][a] + lambda;
  bool ok = true;
  for (int j = 0; j < 6; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k] * D[k];
    D[j] = d;
    if (d <= 0.0) ok = false;
    for (int i = j + 1; i < 6; i++) {
      double s = A[i][j];
      for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
  for (int i = 0; i < 6; i++) {
    double s = -acc[1 + i];  // b = -(the summed J^T Omega e)
    for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
    y[i] = s;
  }
  for (int i = 5; i >= 0; i--) {
    double s = y[i] / D[i];
    for (int k = i + 1; k < 6; k++) s = s - L[k][i] * x[k];
    x[i] = s;
  }
  return ok;
}

// SparseOptimizer::optimize(10) with OptimizationAlgorithmLevenberg.  Team::build / Team::chi evaluate at an estimate over
// the active edges through the fixed tree and leave the result with EVERY caller (the device runs this redundantly on
// every lane).  Returns through *T the estimate after the last accepted step.
template <class Team>
VSG_HD void lm_optimize(Team &tm, Est *T, bool robust) {
  double lambda = 0.0, ni = 2.0;
  int n_bad = 0;
  for (int it = 0; it < kIters; it++) {
    double acc[kAcc];
    tm.build(*T, robust, acc);
    double currentChi = acc[0], tempChi = currentChi;
    const double iniChi = currentChi;
    if (it == 0) {
      double maxDiagonal = 0.0;
      int h = 7;
      for (int a = 0; a < 6; h += 6 - a, a++) {
        const double d = __builtin_fabs(acc[h]);
        maxDiagonal = d < maxDiagonal ? maxDiagonal : d;  // std::max(fabs(v->hessian(j, j)), maxDiagonal)
      }
      lambda = 1e-5 * maxDiagonal;
      ni = 2.0, n_bad = 0;
    }
    double rho = 0.0;
    int qmax = 0;
    for (int trial = 0; trial < kTrials; trial++) {
      double x[6];
      const bool ok2 = solve6(acc, lambda, x);
      const Est cand = est_oplus(*T, x);
      tempChi = tm.chi(cand, robust);
      if (!ok2) tempChi = 1.7976931348623157e308;
      rho = currentChi - tempChi;
      double scale = 0.0;
      for (int j = 0; j < 6; j++) scale = scale + x[j] * (lambda * x[j] + -acc[1 + j]);
      scale = scale + 1e-3;
      rho = rho / scale;
      if (rho > 0 && tempChi - tempChi == 0.0) {  // g2o_isfinite(tempChi)
        const double p = 2 * rho - 1;
        double alpha = 1.0 - p * p * p;
        alpha = 2.0 / 3.0 < alpha ? 2.0 / 3.0 : alpha;          // std::min(alpha, _goodStepUpperScale)
        const double f = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;  // std::max(_goodStepLowerScale, alpha)
        lambda = lambda * f;
        ni = 2.0;
        currentChi = tempChi;
        *T = cand;
      } else {
        lambda = lambda * ni;
        ni = ni * 2.0;
      }
      qmax++;
      if (!(rho < 0)) break;
    }
    if (qmax == kTrials || rho == 0) return;  // Terminate
    if ((iniChi - currentChi) * 1e3 < iniChi)
      n_bad++;
    else
      n_bad = 0;
    if (n_bad >= 3) return;
  }
}

// One edge at the classification of round `it` (:1338-1438).  Returns 1 when the edge counts in nBad; *first_gone = the
// edge left optimizer.edges() just now.
VSG_HD int classify_edge(const Cam &K, const Est &T, Edge *edge, uint8_t *flag, float *chi2_out, int *first_gone) {
  uint8_t f = *flag;
  *first_gone = 0;
  if (f & kOutlier) {
    if (f & kRemoved) {
      if (!(f & kGone)) *first_gone = 1, *flag = (uint8_t)(f | kGone);
      return 1;
    }
    double e[3], Xc[3];
    edge->chi2 = edge_error(K, T, *edge, (f & kStereo) != 0, e, Xc);
  }
  const float chi2 = (float)edge->chi2;
  *chi2_out = canonf(chi2);
  const bool bad = chi2 > ((f & kStereo) ? 7.815f : 5.991f);
  *flag = (uint8_t)(bad ? (f | kOutlier) : (f & ~kOutlier));
  return bad ? 1 : 0;
}

// The round loop (:1254-1442).  mode kModeHold stops after round 2's optimize with C->held = 1; kModeResume starts at
// round 2's classification.  Team::classify runs classify_edge over all edges and returns the two counts to everyone.
template <class Team>
VSG_HD void run_rounds(Team &tm, Ctl *C, int mode) {
  int first = 0;
  if (mode == kModeResume) {
    first = 2;
  } else {
    C->robust = 1, C->edges_left = C->n_edges, C->n_bad = 0, C->rounds_run = 0, C->est = C->input;
  }
  C->held = 0;
  for (int it = first; it < kRounds; it++) {
    if (!(mode == kModeResume && it == 2)) {
      Est T = C->input;  // every round restarts from the frame's pose (:1263)
      lm_optimize(tm, &T, C->robust != 0);
      C->est = T;
      if (mode == kModeHold && it == 2) {
        C->held = 1;
        return;
      }
    }
    if (it == 2) C->robust = 0;
    int n_bad = 0, gone = 0;
    tm.classify(C->est, &n_bad, &gone);
    C->n_bad = n_bad, C->edges_left -= gone, C->rounds_run = it + 1;
    if (C->edges_left < 10) break;
  }
}

// ---- the host's Team: replays the device's tree thread by thread
struct HostTeam {
  Cam K;
  Edge *edges;
  uint8_t *flags;
  float *chi2_out;  // per edge
  int n_edges;

  template <int W>  // W accumulators per thread: kAcc here, 36 in vsg_sim3_opt.h, one tree
  static void tree(double (*part)[W], int n, double *acc) {
    for (int k = 0; k < n; k++) {
      double wave_sum[kWaves];
      for (int w = 0; w < kWaves; w++) {
        double v[kWave], o[kWave];
        for (int l = 0; l < kWave; l++) v[l] = part[w * kWave + l][k];
        for (int s = 1; s < kWave; s <<= 1) {
          for (int l = 0; l < kWave; l++) o[l] = v[l] + v[l ^ s];
          for (int l = 0; l < kWave; l++) v[l] = o[l];
        }
        wave_sum[w] = v[0];
      }
      double t = wave_sum[0];
      for (int w = 1; w < kWaves; w++) t = t + wave_sum[w];
      acc[k] = t;
    }
  }
  void eval(const Est &T, bool robust, bool build_it, double *acc) {
    static thread_local double part[kThreads][kAcc];
    for (int t = 0; t < kThreads; t++) thread_partial(K, T, edges, flags, n_edges, t, robust, build_it, part[t]);
    tree(part, build_it ? (int)kAcc : 1, acc);
  }
  void build(const Est &T, bool robust, double *acc) { eval(T, robust, true, acc); }
  double chi(const Est &T, bool robust) {
    double c;
    eval(T, robust, false, &c);
    return c;
  }
  void classify(const Est &T, int *n_bad, int *gone) {
    for (int i = 0; i < n_edges; i++) {
      int g = 0;
      *n_bad += classify_edge(K, T, &edges[i], &flags[i], &chi2_out[i], &g);
      *gone += g;
    }
  }
};

// ---- the whole call on the host, as vsg_pose.hip stages it: the argument check, the gather, the rounds, the copy-out

// the slots and octaves of a call; *n_edges = the features with a slot.  false: a slot >= capacity, or a feature with a
// slot whose octave is >= nlevels (octave(i) is asked only for i < n_octaves)
template <class OctaveOf>
inline bool check_slots(int n, const int32_t *feat_slots, int capacity, int nlevels, int n_octaves, OctaveOf octave,
                        int *n_edges) {
  int E = 0;
  for (int i = 0; i < n; i++) {
    if (feat_slots[i] < 0) continue;
    if (feat_slots[i] >= capacity) return false;
    if (i < n_octaves && octave(i) >= nlevels) return false;
    E++;
  }
  *n_edges = E;
  return true;
}

struct HostCall {
  std::vector<Edge> edges;
  std::vector<uint8_t> flags;
  std::vector<float> chi2;
  std::vector<int32_t> feat;
  Ctl ctl;

  // :1109-1180 for the features with a slot, in feature order
  void gather(int n, const int32_t *feat_slots, const float *world_pos, const float *kx, const float *ky,
              const int32_t *octave, const float *u_right, const float *inv_level_sigma2, int nlevels, const Cam &cam,
              const Est &input) {
    edges.clear(), flags.clear(), chi2.clear(), feat.clear();
    for (int i = 0; i < n; i++) {
      if (feat_slots[i] < 0) continue;
      const size_t s = (size_t)feat_slots[i];
      const float ur = u_right ? u_right[i] : -1.0f;
      const bool stereo = !(ur < 0);
      const int o = octave[i] & 15;
      Edge e;
      e.X[0] = (double)world_pos[3 * s], e.X[1] = (double)world_pos[3 * s + 1], e.X[2] = (double)world_pos[3 * s + 2];
      e.obs[0] = (double)kx[i], e.obs[1] = (double)ky[i], e.obs[2] = stereo ? (double)ur : 0.0;
      e.w = (double)inv_level_sigma2[o < nlevels ? o : nlevels - 1];
      e.chi2 = 0.0;
      edges.push_back(e), flags.push_back(stereo ? kStereo : 0), chi2.push_back(0.0f), feat.push_back(i);
    }
    ctl.cam = cam, ctl.input = input, ctl.n_edges = (int)edges.size();
  }
  void remove(const uint8_t *removed) {
    if (!removed) return;
    for (size_t e = 0; e < edges.size(); e++)
      if (removed[feat[e]]) flags[e] = (uint8_t)(flags[e] | kOutlier | kRemoved);
  }
  void rounds(int mode) {
    HostTeam tm = {ctl.cam, edges.data(), flags.data(), chi2.data(), (int)edges.size()};
    run_rounds(tm, &ctl, mode);
  }
  void copy_out(uint8_t *outlier, float *chi2_out) const {
    for (size_t e = 0; e < edges.size(); e++) {
      outlier[feat[e]] = (flags[e] & kOutlier) ? 1 : 0;
      if (chi2_out) chi2_out[feat[e]] = chi2[e];
    }
  }
};

}  // namespace pose
}  // namespace vsg
