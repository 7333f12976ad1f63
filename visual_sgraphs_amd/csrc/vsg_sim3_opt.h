// vsg_sim3_opt.h -- Optimizer::OptimizeSim3 (Optimizer.cc:3261-3529) for ONE pair of keyframes, host and device from one
// source: k_sim3_optimize (vsg_sim3_opt.hip) runs it as one persistent workgroup, tests/_sim3optcore and the latency
// probe's caller-side path (tools/resident_points_cpu.cpp) compile it for the host.  The pattern is vsg_pose_opt.h's, which
// this file includes for sincos_pose, the quaternion helpers, huber, canon and the reduction tree.
//
// Everything is double, as g2o has it, but the pair set-up, which the reference does in float (:3335, :3343, :3421-3423).
// What is restated, and from where:
//   * the vertex: VertexSim3Expmap::oplusImpl (OptimizableTypes.h:172-181) with _fix_scale zeroing update[6] IN THE
//     CALLER'S ARRAY, g2o::Sim3's exponential, map, inverse and operator* (sim3.h:67-134, :136-139, :219-222, :254-261;
//     operator* does NOT normalise the quaternion and setEstimate takes the input as it is);
//   * the two edges: EdgeSim3ProjectXYZ and EdgeInverseSim3ProjectXYZ (OptimizableTypes.h:196-221) through
//     Pinhole::project(Vector3d) (Pinhole.cpp:37-44);
//   * the NUMERIC Jacobian of BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-205): neither edge defines its
//     own, so each of the 7 columns is (1 / (2 delta)) * (e(+delta e_d) - e(-delta e_d)) with delta = 1e-9, the point
//     vertices being fixed.  The 14 perturbed estimates exp(+-delta e_d) * estimate and their inverses depend on the
//     estimate alone: they are computed ONCE per build pass (perturbed below), not per edge;
//   * BaseBinaryEdge::constructQuadraticForm for the one free vertex (base_binary_edge.hpp:73-113), the robust branch in
//     the first optimisation and the plain one in the second (setRobustKernel(0), :3484-3485);
//   * OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale (optimization_algorithm_levenberg.cpp:
//     61-194) at dimension 7, the sibling of pose::lm_optimize (which stays as it is: PoseOptimization must not change
//     by a bit), with the dense solve as an LDL^T without pivoting;
//   * the two checks, the gate and the return (:3452-3528).
//
// Both builds use -ffp-contract=off.  exp is written out here (exp_sim3: exp(+-1e-9) decides column 6 of every
// Jacobian), sin / cos are pose::sincos_pose.
//
// SUMS OVER EDGES use the tree of vsg_pose_opt.h.  Pair p -- its two edges, e12 first -- belongs to lane p % kThreads in
// every pass; the pairs are the CANDIDATES (both points present) in feature order, and one that the set-up skipped
// (z < 0, i2 < 0) simply is not active, so nothing is compacted on the device.
//
// Every loop has a compile-time bound (2 optimisations, at most 10 iterations, 10 trials, 7 columns x 2 signs).
#pragma once
#include <stdint.h>

#include <vector>

#include "vsg_pose_opt.h"
#include "vsg_sim3.h"

#if defined(__HIPCC__)
#define VSG_S3O_UNROLL _Pragma("unroll")
#else
#define VSG_S3O_UNROLL
#endif

namespace vsg {
namespace sim3opt {

enum { kThreads = pose::kThreads, kDim = 7, kAcc = 1 + kDim + kDim * (kDim + 1) / 2, kIters = 10, kTrials = 10, kPert = 2 * kDim };
// state[i] of include/vsg_orb.h
enum { kNoEdge = 0, kInlier = 1, kBadFirst = 2, kBadSecond = 3, kSkipZ = 4, kSkipI2 = 5 };

struct Sim3 {
  double q[4], t[3], s;  // g2o::Sim3: r as x y z w (NOT normalised by anything here), t, s
};
struct Cams {
  double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;  // pCamera1 / pCamera2: the keyframes' floats, widened
};
// one candidate pair: 112 bytes.  chi12 / chi21 = the edges' chi2() as the last computeError left them (the STALE-error
// rule of the first check lives here)
struct Pair {
  double X1[3], X2[3], obs1[2], obs2[2], w1, w2, chi12, chi21;
};
// the perturbed estimates of one build pass: entry 2 d + (0: +delta, 1: -delta)
struct Pert {
  Sim3 fwd[kPert], inv[kPert];
};

VSG_HD Cams cams_of(const vsg_frame_pose &kf1, const vsg_frame_pose &kf2) {
  return Cams{(double)kf1.fx, (double)kf1.fy, (double)kf1.cx, (double)kf1.cy,
              (double)kf2.fx, (double)kf2.fy, (double)kf2.cx, (double)kf2.cy};
}

// ---- exp for Sim3(Vector7d)'s `s = std::exp(sigma)`: fdlibm's e_exp.c on [-1, 1] (k = 0 below 0.5 ln 2, else k = +-1),
// WITHOUT its |x| < 2^-28 shortcut 1 + x, which misses the x^2 / 2 that decides a rounding of exp(1e-9) now and then.
// The CPU test measures it against libm: equal for |x| <= 1e-8, within 1 ulp on [-1, 1].  Outside of [-1, 1], or NaN:
// NaN (the update is then NaN and the trial is rejected).
VSG_HD double exp_sim3(double x) {
  if (!(x >= -1.0 && x <= 1.0)) return __builtin_nan("");
  const double ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10, P1 = 1.66666666666666019037e-01,
               P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05, P4 = -1.65339022054652515390e-06,
               P5 = 4.13813679705723846039e-08;
  double hi = x, lo = 0.0;
  int k = 0;
  if (__builtin_fabs(x) > 0.34657359027997264) {  // 0.5 ln 2; |x| <= 1 < 1.5 ln 2, so k = +-1
    k = x < 0 ? -1 : 1;
    hi = x - (double)k * ln2HI;
    lo = (double)k * ln2LO;
    x = hi - lo;
  }
  const double t = x * x;
  const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
  if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
  const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
  return k == 1 ? y * 2.0 : y * 0.5;
}

// ---- g2o::Sim3
VSG_HD Sim3 sim3_exp(const double *u) {  // Sim3(const Vector7d &update): update = [omega, upsilon, sigma]
  const double sigma = u[6];
  const double theta = sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2]);
  const double O[3][3] = {{0.0, -u[2], u[1]}, {u[2], 0.0, -u[0]}, {-u[1], u[0], 0.0}};
  double O2[3][3], R[3][3];
  VSG_S3O_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_S3O_UNROLL
    for (int j = 0; j < 3; j++) O2[i][j] = (O[i][0] * O[0][j] + O[i][1] * O[1][j]) + O[i][2] * O[2][j];
  Sim3 S;
  S.s = exp_sim3(sigma);
  const double eps = 0.00001;
  const bool small_theta = theta < eps;
  double A, B, C, sn = 0.0, cs = 1.0;
  if (!small_theta) pose::sincos_pose(theta, &sn, &cs);
  if (small_theta) {
    VSG_S3O_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_S3O_UNROLL
      for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + O[i][j]) + O2[i][j];
  } else {
    const double a = sn / theta, b = (1 - cs) / (theta * theta);
    VSG_S3O_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_S3O_UNROLL
      for (int j = 0; j < 3; j++) R[i][j] = ((i == j ? 1.0 : 0.0) + a * O[i][j]) + b * O2[i][j];
  }
  if (__builtin_fabs(sigma) < eps) {
    C = 1;
    if (small_theta) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (S.s - 1) / sigma;
    if (small_theta) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * S.s + 1) / sigma2;
      B = ((0.5 * sigma2 - sigma + 1) * S.s) / (sigma2 * sigma);
    } else {
      const double a = S.s * sn, b = S.s * cs, theta2 = theta * theta, sigma2 = sigma * sigma;
      const double c = theta2 + sigma2;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  pose::quat_from_matrix(R, S.q);  // r = Quaterniond(R): not normalised
  VSG_S3O_UNROLL
  for (int i = 0; i < 3; i++) {
    double W[3];
    VSG_S3O_UNROLL
    for (int j = 0; j < 3; j++) W[j] = (A * O[i][j] + B * O2[i][j]) + C * (i == j ? 1.0 : 0.0);
    S.t[i] = (W[0] * u[3] + W[1] * u[4]) + W[2] * u[5];
  }
  return S;
}
VSG_HD void sim3_map(const Sim3 &S, const double *x, double *o) {  // s * (r * xyz) + t
  double r[3];
  pose::quat_rotate(S.q, x, r);
  o[0] = S.s * r[0] + S.t[0], o[1] = S.s * r[1] + S.t[1], o[2] = S.s * r[2] + S.t[2];
}
VSG_HD Sim3 sim3_mul(const Sim3 &a, const Sim3 &b) {  // operator*: r * other.r, s * (r * other.t) + t, s * other.s
  Sim3 o;
  pose::quat_mul(a.q, b.q, o.q);
  sim3_map(a, b.t, o.t);
  o.s = a.s * b.s;
  return o;
}
VSG_HD Sim3 sim3_inverse(const Sim3 &a) {  // Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
  Sim3 o;
  o.q[0] = -a.q[0], o.q[1] = -a.q[1], o.q[2] = -a.q[2], o.q[3] = a.q[3];
  const double f = -1. / a.s;
  const double v[3] = {f * a.t[0], f * a.t[1], f * a.t[2]};
  pose::quat_rotate(o.q, v, o.t);
  o.s = 1. / a.s;
  return o;
}
// oplusImpl: `if (_fix_scale) update[6] = 0` in the caller's array, then setEstimate(Sim3(update) * estimate())
VSG_HD Sim3 sim3_oplus(const Sim3 &cur, double *u, bool fix_scale) {
  if (fix_scale) u[6] = 0;
  return sim3_mul(sim3_exp(u), cur);
}
// perturbed estimate k = 2 d + sign of linearizeOplus (:157-170) and its inverse (what EdgeInverseSim3ProjectXYZ maps by)
VSG_HD void perturbed(const Sim3 &cur, int k, bool fix_scale, Sim3 *fwd, Sim3 *inv) {
  const double delta = 1e-9;
  double u[kDim];
  VSG_S3O_UNROLL
  for (int d = 0; d < kDim; d++) u[d] = d == (k >> 1) ? ((k & 1) ? -delta : delta) : 0.0;
  *fwd = sim3_oplus(cur, u, fix_scale);
  *inv = sim3_inverse(*fwd);
}

// ---- the pair set-up (:3313-3450) for one candidate, in FLOAT as the reference has it.  Returns the state: kSkipI2
// (`i2 < 0 && !bAllPoints`, tested first), kSkipZ (`P3D2c(2) < 0`) or kInlier with *P filled.  kp2 / oct2 = KF2's
// mvKeysUn[i2] when i2 >= 0; otherwise oct2 = pMP2->mnTrackScaleLevel and the observation is the NORMALISED coordinate
// (P3D2c.x * invz, P3D2c.y * invz) with invz = 1 / P3D2c.z, all float -- not a pixel (:3421-3426), kept.
VSG_HD int make_pair(const vsg_frame_pose &kf1, const vsg_frame_pose &kf2, const float *Xw1, const float *Xw2, float k1x,
                     float k1y, int oct1, int i2, float k2x, float k2y, int oct2, const float *inv_sigma2_1,
                     const float *inv_sigma2_2, bool all_points, Pair *P) {
  if (i2 < 0 && !all_points) return kSkipI2;
  float X1c[3], X2c[3];
  sim3::camera_point(kf1, Xw1, X1c), sim3::camera_point(kf2, Xw2, X2c);
  if (X2c[2] < 0) return kSkipZ;
  VSG_S3O_UNROLL
  for (int k = 0; k < 3; k++) P->X1[k] = (double)X1c[k], P->X2[k] = (double)X2c[k];
  P->obs1[0] = (double)k1x, P->obs1[1] = (double)k1y;
  P->w1 = (double)inv_sigma2_1[oct1 & 15];
  if (i2 >= 0) {
    P->obs2[0] = (double)k2x, P->obs2[1] = (double)k2y;
  } else {
    const float invz = fdiv(1.0f, X2c[2]);
    P->obs2[0] = (double)fmul(X2c[0], invz), P->obs2[1] = (double)fmul(X2c[1], invz);
  }
  P->w2 = (double)inv_sigma2_2[oct2 & 15];
  P->chi12 = P->chi21 = 0.0;
  return kInlier;
}

// ---- the edges.  computeError + chi2(): obs - project(S.map(X)); information = invSigma2 * I multiplied out with its
// zeros as Eigen does.  S = the estimate for e12 (with X2c, camera 1), its INVERSE for e21 (with X1c, camera 2).
VSG_HD void edge_error(double fx, double fy, double cx, double cy, const Sim3 &S, const double *X, const double *obs,
                       double *e) {
  double Xc[3];
  sim3_map(S, X, Xc);
  e[0] = obs[0] - (fx * Xc[0] / Xc[2] + cx);
  e[1] = obs[1] - (fy * Xc[1] / Xc[2] + cy);
}
VSG_HD double edge_chi2(const double *e, double w) { return e[0] * (w * e[0] + 0.0 * e[1]) + e[1] * (0.0 * e[0] + w * e[1]); }
VSG_HD void error12(const Cams &K, const Sim3 &S, const Pair &P, double *e) { edge_error(K.fx1, K.fy1, K.cx1, K.cy1, S, P.X2, P.obs1, e); }
VSG_HD void error21(const Cams &K, const Sim3 &Sinv, const Pair &P, double *e) { edge_error(K.fx2, K.fy2, K.cx2, K.cy2, Sinv, P.X1, P.obs2, e); }

// constructQuadraticForm of one edge into acc: acc[1 + a] += (B^T omega_r)[a] with omega_r = -(Omega e) [* rho1],
// acc[8 ..] += the upper triangle of B^T (rho1 Omega) B.  rho1 = 1 is the plain branch (a multiplication by 1 is exact).
VSG_HD void quadratic_form(const double J[2][kDim], const double *e, double w, double rho1, double *acc) {
  const double r0 = -(w * e[0] + 0.0 * e[1]) * rho1, r1 = -(0.0 * e[0] + w * e[1]) * rho1;
  const double wo = rho1 * w;
  int h = 1 + kDim;
  VSG_S3O_UNROLL
  for (int a = 0; a < kDim; a++) {
    acc[1 + a] = acc[1 + a] + (J[0][a] * r0 + J[1][a] * r1);
    VSG_S3O_UNROLL
    for (int c = a; c < kDim; c++, h++) acc[h] = acc[h] + ((J[0][a] * wo) * J[0][c] + (J[1][a] * wo) * J[1][c]);
  }
}

// One thread's part of an evaluation: its pairs tid, tid + kThreads, ... in that order, e12 before e21.  Only pairs in
// state kInlier are active.  BUILD: acc[0] = activeRobustChi2's part, acc[1..7] the part of b, acc[8..35] the upper
// triangle of H row by row; else acc[0] alone.  Both store the edges' chi2.  pert = the perturbed estimates of S.
template <bool BUILD>
VSG_HD void thread_partial(const Cams &K, const Sim3 &S, const Pert *pert, Pair *pairs, const uint8_t *state, int n_pairs,
                           int tid, bool robust, double delta, double *acc) {
  VSG_S3O_UNROLL
  for (int k = 0; k < (BUILD ? (int)kAcc : 1); k++) acc[k] = 0.0;
  const Sim3 Sinv = sim3_inverse(S);
  const double scalar = 1.0 / (2 * 1e-9);
  for (int p = tid; p < n_pairs; p += kThreads) {
    if (state[p] != kInlier) continue;
    const Pair P = pairs[p];
    double e12[2], e21[2];
    error12(K, S, P, e12), error21(K, Sinv, P, e21);
    const double c12 = edge_chi2(e12, P.w1), c21 = edge_chi2(e21, P.w2);
    pairs[p].chi12 = c12, pairs[p].chi21 = c21;
    double a12 = c12, b12 = 1.0, a21 = c21, b21 = 1.0;
    if (robust) pose::huber(c12, delta, &a12, &b12), pose::huber(c21, delta, &a21, &b21);
    acc[0] = acc[0] + a12;
    acc[0] = acc[0] + a21;
    if constexpr (BUILD) {
    double J[2][kDim];
    VSG_S3O_UNROLL
    for (int d = 0; d < kDim; d++) {
      double ep[2], em[2];
      error12(K, pert->fwd[2 * d], P, ep), error12(K, pert->fwd[2 * d + 1], P, em);
      J[0][d] = scalar * (ep[0] - em[0]), J[1][d] = scalar * (ep[1] - em[1]);
    }
    quadratic_form(J, e12, P.w1, b12, acc);
    VSG_S3O_UNROLL
    for (int d = 0; d < kDim; d++) {
      double ep[2], em[2];
      error21(K, pert->inv[2 * d], P, ep), error21(K, pert->inv[2 * d + 1], P, em);
      J[0][d] = scalar * (ep[0] - em[0]), J[1][d] = scalar * (ep[1] - em[1]);
    }
    quadratic_form(J, e21, P.w2, b21, acc);
    }
  }
}

// (H + lambda I) x = b by LDL^T without pivoting, as pose::solve6 at dimension 7 (b is stored with its own sign here)
VSG_HD bool solve7(const double *acc, double lambda, double *x) {
  double A[kDim][kDim], L[kDim][kDim], D[kDim], y[kDim];
  int h = 1 + kDim;
  for (int a = 0; a < kDim; a++)
    for (int c = a; c < kDim; c++, h++) A[a][c] = A[c][a] = acc[h];
  for (int a = 0; a < kDim; a++) A[a][a] = A[a][a] + lambda;
  bool ok = true;
  for (int j = 0; j < kDim; j++) {
    double d = A[j][j];
    for (int k = 0; k < j; k++) d = d - L[j][k] * L[j][k] * D[k];
    D[j] = d;
    if (d <= 0.0) ok = false;
    for (int i = j + 1; i < kDim; i++) {
      double s = A[i][j];
      for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
      L[i][j] = s / d;
    }
  }
  for (int i = 0; i < kDim; i++) {
    double s = acc[1 + i];
    for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
    y[i] = s;
  }
  for (int i = kDim - 1; i >= 0; i--) {
    double s = y[i] / D[i];
    for (int k = i + 1; k < kDim; k++) s = s - L[k][i] * x[k];
    x[i] = s;
  }
  return ok;
}

// SparseOptimizer::optimize(iterations) with OptimizationAlgorithmLevenberg: pose::lm_optimize at dimension 7, with the
// iteration count of the call (5, or 10) and oplusImpl's zeroing of x[6], which computeScale then reads.
template <class Team>
VSG_HD void lm_optimize(Team &tm, Sim3 *T, bool robust, int iterations, bool fix_scale) {
  double lambda = 0.0, ni = 2.0;
  int n_bad = 0;
  for (int it = 0; it < kIters && it < iterations; it++) {
    double acc[kAcc];
    tm.build(*T, robust, acc);
    double currentChi = acc[0], tempChi = currentChi;
    const double iniChi = currentChi;
    if (it == 0) {
      double maxDiagonal = 0.0;
      int h = 1 + kDim;
      for (int a = 0; a < kDim; h += kDim - a, a++) {
        const double d = __builtin_fabs(acc[h]);
        maxDiagonal = d < maxDiagonal ? maxDiagonal : d;  // std::max(fabs(v->hessian(j, j)), maxDiagonal)
      }
      lambda = 1e-5 * maxDiagonal;
      ni = 2.0, n_bad = 0;
    }
    double rho = 0.0;
    int qmax = 0;
    for (int trial = 0; trial < kTrials; trial++) {
      double x[kDim];
      const bool ok2 = solve7(acc, lambda, x);
      const Sim3 cand = sim3_oplus(*T, x, fix_scale);
      tempChi = tm.chi(cand, robust);
      if (!ok2) tempChi = 1.7976931348623157e308;
      rho = currentChi - tempChi;
      double scale = 0.0;
      for (int j = 0; j < kDim; j++) scale = scale + x[j] * (lambda * x[j] + acc[1 + j]);
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

// One pair at a check.  first (:3459-3486): the chi2 the LAST computeActiveErrors left; second (:3503-3522):
// computeError() fresh at the estimate.  A pair is bad when EITHER chi2 > th2 (a double against the widened float).
// Returns 1 for a pair that was active and is bad now.
VSG_HD int check_pair(const Cams &K, const Sim3 &S, const Sim3 &Sinv, Pair *P, uint8_t *state, double th2, bool fresh,
                      int bad_state) {
  if (*state != kInlier) return 0;
  if (fresh) {
    double e12[2], e21[2];
    error12(K, S, *P, e12), error21(K, Sinv, *P, e21);
    P->chi12 = edge_chi2(e12, P->w1), P->chi21 = edge_chi2(e21, P->w2);
  }
  if (P->chi12 > th2 || P->chi21 > th2) {
    *state = (uint8_t)bad_state;
    return 1;
  }
  return 0;
}

struct Outcome {
  Sim3 S12;  // g2oS12 on return
  int n_bad, n_in, more_iterations, updated, ret;
};

// :3452-3528.  Team::check runs check_pair over all pairs and returns the count of bad ones to everyone.  FIRST_FRESH is
// NOT the reference: it recomputes the errors at the first check too, so that a test can show on the same arithmetic
// that the stale rule decides bits (tests/_sim3optcore); the library never sets it.
template <bool FIRST_FRESH = false, class Team>
VSG_HD Outcome run(Team &tm, const Sim3 &input, int n_correspondences, double th2, bool fix_scale) {
  Outcome o;
  o.S12 = input, o.n_bad = 0, o.n_in = 0, o.more_iterations = 5, o.updated = 0, o.ret = 0;
  Sim3 est = input;
  for (int opt = 0; opt < 2; opt++) {  // one call site: the device inlines the whole optimisation once
    // optimize() returns at once without an edge; the second one starts again at iteration 0 (lambda is re-initialised)
    if (n_correspondences > 0) lm_optimize(tm, &est, opt == 0, opt == 0 ? 5 : o.more_iterations, fix_scale);
    const int bad = tm.check(est, th2, opt == 1 || FIRST_FRESH, opt == 1 ? kBadSecond : kBadFirst);
    if (opt == 0) {
      o.n_bad = bad;
      o.more_iterations = bad > 0 ? 10 : 5;
      if (n_correspondences - bad < 10) return o;  // g2oS12 is NOT updated; the bad matches are already nulled
    } else {
      o.n_in = n_correspondences - o.n_bad - bad;
      o.S12 = est, o.updated = 1, o.ret = o.n_in;
    }
  }
  return o;
}

VSG_HD Sim3 sim3_of(const vsg_sim3d &s) {
  Sim3 o;
  for (int k = 0; k < 4; k++) o.q[k] = s.q[k];
  for (int k = 0; k < 3; k++) o.t[k] = s.t[k];
  o.s = s.s;
  return o;
}
VSG_HD vsg_sim3d sim3d_canon(const Sim3 &s) {
  vsg_sim3d o;
  for (int k = 0; k < 4; k++) o.q[k] = pose::canon(s.q[k]);
  for (int k = 0; k < 3; k++) o.t[k] = pose::canon(s.t[k]);
  o.s = pose::canon(s.s);
  return o;
}
// deltaHuber = sqrt(th2) stored in a float (:3303); RobustKernelHuber::setDelta widens it
inline double huber_delta_of(float th2) { return (double)(float)sqrt((double)th2); }

// ---- the host's Team: replays the device's tree thread by thread
struct HostTeam {
  Cams K;
  Pair *pairs;
  uint8_t *state;
  int n_pairs;
  double delta;
  bool fix_scale;
  Pert pert;

  void eval(const Sim3 &S, bool robust, bool build_it, double *acc) {
    static thread_local double part[kThreads][kAcc];
    if (build_it)
      for (int k = 0; k < kPert; k++) perturbed(S, k, fix_scale, &pert.fwd[k], &pert.inv[k]);
    for (int t = 0; t < kThreads; t++) {
      if (build_it)
        thread_partial<true>(K, S, &pert, pairs, state, n_pairs, t, robust, delta, part[t]);
      else
        thread_partial<false>(K, S, &pert, pairs, state, n_pairs, t, robust, delta, part[t]);
    }
    pose::HostTeam::tree(part, build_it ? (int)kAcc : 1, acc);
  }
  void build(const Sim3 &S, bool robust, double *acc) { eval(S, robust, true, acc); }
  double chi(const Sim3 &S, bool robust) {
    double c;
    eval(S, robust, false, &c);
    return c;
  }
  int check(const Sim3 &S, double th2, bool fresh, int bad_state) {
    const Sim3 Sinv = sim3_inverse(S);
    int bad = 0;
    for (int p = 0; p < n_pairs; p++) bad += check_pair(K, S, Sinv, &pairs[p], &state[p], th2, fresh, bad_state);
    return bad;
  }
};

// ---- the whole call on the host, as vsg_sim3_opt.hip stages it: the argument check, the gather, the run, the copy-out

// The entries of a call.  A candidate is an entry with both slots >= 0; *n_cand counts them.  false: a slot >= its store's
// capacity, or on a candidate: idx2 >= n2, or -- unless `i2 < 0 && !all_points` skips it -- KF1's octave, and KF2's
// octave (idx2 >= 0) or level2 (idx2 < 0), outside [0, nlevels).  oct1(i) / oct2(i2) return the keypoint's octave.
template <class Oct1, class Oct2>
inline bool check_entries(int n, const int32_t *slots1, const int32_t *slots2, const int32_t *idx2, const int32_t *level2,
                          int cap1, int cap2, int n2, int nlevels, bool all_points, Oct1 oct1, Oct2 oct2, int *n_cand) {
  int c = 0;
  for (int i = 0; i < n; i++) {
    if (slots1[i] >= cap1 || slots2[i] >= cap2) return false;
    if (slots1[i] < 0 || slots2[i] < 0) continue;
    c++;
    const int i2 = idx2[i];
    if (i2 >= n2) return false;
    if (i2 < 0 && !all_points) continue;
    const int o1 = oct1(i), o2 = i2 >= 0 ? oct2(i2) : level2[i];
    if (o1 < 0 || o1 >= nlevels || o2 < 0 || o2 >= nlevels) return false;
  }
  *n_cand = c;
  return true;
}
inline bool th2_ok(float th2) { return th2 - th2 == 0.0f && th2 > 0.0f; }  // finite and positive

// what the gather counts
struct Counts {
  int n_correspondences, n_in_kf2, n_out_kf2;
};

struct HostCall {
  std::vector<Pair> pairs;
  std::vector<uint8_t> state;
  std::vector<int32_t> feat;
  Counts counts;

  // kps1 / kps2: x, y per feature; oct1 / oct2: the octaves; pos1 / pos2: the stores' GetWorldPos()
  void gather(int n, const int32_t *slots1, const int32_t *slots2, const int32_t *idx2, const int32_t *level2,
              const float *pos1, const float *pos2, const float *k1x, const float *k1y, const int32_t *oct1,
              const float *k2x, const float *k2y, const int32_t *oct2, const vsg_frame_pose &kf1, const vsg_frame_pose &kf2,
              const float *sig1, const float *sig2, int nlevels, bool all_points) {
    float t1[16], t2[16];
    for (int l = 0; l < 16; l++) t1[l] = sig1[l < nlevels ? l : nlevels - 1], t2[l] = sig2[l < nlevels ? l : nlevels - 1];
    pairs.clear(), state.clear(), feat.clear();
    counts = Counts{0, 0, 0};
    for (int i = 0; i < n; i++) {
      if (slots1[i] < 0 || slots2[i] < 0) continue;
      const int i2 = idx2[i];
      Pair P = {};
      const int st = make_pair(kf1, kf2, pos1 + 3 * (size_t)slots1[i], pos2 + 3 * (size_t)slots2[i], k1x[i], k1y[i], oct1[i], i2,
                               i2 >= 0 ? k2x[i2] : 0.0f, i2 >= 0 ? k2y[i2] : 0.0f, i2 >= 0 ? oct2[i2] : level2[i], t1, t2,
                               all_points, &P);
      pairs.push_back(P), state.push_back((uint8_t)st), feat.push_back(i);
      if (st == kInlier) counts.n_correspondences++, (i2 >= 0 ? counts.n_in_kf2 : counts.n_out_kf2)++;
    }
  }
  Outcome optimise(const vsg_frame_pose &kf1, const vsg_frame_pose &kf2, const Sim3 &input, float th2, bool fix_scale,
                   bool first_fresh = false) {
    HostTeam tm = {cams_of(kf1, kf2), pairs.data(), state.data(), (int)pairs.size(), huber_delta_of(th2), fix_scale, {}};
    if (first_fresh) return run<true>(tm, input, counts.n_correspondences, (double)th2, fix_scale);
    return run(tm, input, counts.n_correspondences, (double)th2, fix_scale);
  }
  // state[i] for ALL i of the n features; chi2 only for the pairs with an edge
  void copy_out(int n, uint8_t *state_out, double *chi2) const {
    for (int i = 0; i < n; i++) state_out[i] = kNoEdge;
    for (size_t p = 0; p < pairs.size(); p++) {
      const uint8_t st = state[p];
      state_out[feat[p]] = st;
      if (chi2 && st >= kInlier && st <= kBadSecond)
        chi2[2 * (size_t)feat[p]] = pose::canon(pairs[p].chi12), chi2[2 * (size_t)feat[p] + 1] = pose::canon(pairs[p].chi21);
    }
  }
};

inline void fill_result(vsg_sim3_opt_result *res, const vsg_sim3d &S12, const Counts &c, int n_bad, int n_in,
                        int more_iterations, int updated) {
  res->S12 = S12;
  res->n_correspondences = c.n_correspondences, res->n_bad = n_bad, res->n_in = n_in, res->n_in_kf2 = c.n_in_kf2;
  res->n_out_kf2 = c.n_out_kf2, res->more_iterations = more_iterations, res->updated = updated;
}

}  // namespace sim3opt
}  // namespace vsg
