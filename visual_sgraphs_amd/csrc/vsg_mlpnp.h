// vsg_mlpnp.h -- MLPnPsolver (MLPnPsolver.cpp) on 2D-3D correspondences of one frame, host and device from one source: the
// constructor's set-up of one correspondence (:76-90, :266), computePose on a set of correspondences (:365-683) with its
// Gauss-Newton (:720-788), CheckInliers (:269-301), and the selection over the hypotheses' inlier counts that iterate's
// loop (:104-229) amounts to.  k_mlpnp_* (vsg_mlpnp.hip) run it on the device, tests/_mlpnpcore
// compiles it for the host.  Both builds use -ffp-contract=off, so every operator below is one IEEE 754 rounding on either
// side (as vsg_pose_opt.h); division and sqrt are the language's, correctly rounded on both sides; sin / cos are
// pose::sincos_pose, acos and the cube root are written out below in a fixed number of steps.
//
// Hypothesis k depends on its six sampled correspondences alone.  WHAT Refine() (:303-362) DOES: it runs computePose over
// the best set into a LOCAL `result` and never copies it into mRi / mti, which only :157-171 write.  The CheckInliers() at
// :340 therefore evaluates hypothesis k's own pose once more: the "refined" count is c[k], Refine() succeeds iff
// c[k] > mRansacMinInliers, and mRefinedTcw / mvbRefinedInliers are hypothesis k's pose and flags.  The solve over the best
// set changes nothing the caller can see, so the library does not run it; the outcome of iterate is a function of the counts
// alone (select below).  member_pose_host restates that discarded solve for the caller-side path of the latency probe and for
// the CPU test of computePose on large sets; no kernel calls it.
//
// SUMS OVER A SET go through a Team: the six samples of a hypothesis are summed serially in drawing order by whoever computes
// the hypothesis (SerialTeam); MemberTeam (host only) sums the members of a set in index order.
//
// DEVIATIONS of arithmetic class, all by rounding unless said otherwise:
//   1. the nullspace pair of a bearing f = (x, y, 1) is Eigen's JacobiSVD basis in the reference.  Here: columns 0 and 1 of
//      the Householder reflection that maps f onto -|f| e_z.  Any orthonormal pair gives the same A^T A and J^T J.
//   2. the null vector of A^T A (12 x 12, planar 9 x 9) and the nearest rotation (3 x 3) come from the one-sided Jacobi of
//      vsg_jacobi.h instead of Eigen's two-sided JacobiSVD; the planar case's eigenvectors from the same routine, sorted by
//      ascending eigenvalue (the lower column on a tie), each signed so that its largest component (the first of equals) is
//      positive -- Eigen's closed-form 3 x 3 solver fixes no sign.
//   3. A^T A and J^T J are summed in the Team's order, not Eigen's product kernels'.
//   4. the 6 x 6 system is solved by an LDL^T WITHOUT pivoting (Eigen's LDLT pivots on the diagonal).
//   5. Ts[s].inverse() (:649) is the rigid inverse (R^T, -R^T t), not Eigen's general 4 x 4 inverse.
//   6. the Jacobian is the analytic one: d/dt = n^T (I - v v^T) / |p| and, through Rodrigues' formula,
//      dR/dw_i = (w_i [w]x + [w x (I - R) e_i]x) R / |w|^2.  AT w = 0 (|w| <= DBL_EPSILON, where rodrigues2rot returns the
//      identity) it takes the limit dR/dw_i = [e_i]x; the reference's generated expression divides by |w| there.
//   7. max|J dx| (:776) ignores NaN entries (the maximum starts at 0); Eigen's maxCoeff keeps a NaN only in entry 0.  Either
//      way the step is applied, and a NaN in J has made dx NaN before.
// KEPT as written: the planarity test on the UNCENTRED points3 * points3^T with Eigen's full-pivot rank threshold; the
// planar scale from columns 1 and 2 of the TRANSPOSED matrix (:565); the direction tests over the first six correspondences
// with the UNNORMALISED bearing; acos of a trace that rounding pushed out of range = NaN, so omega = 0; the aborted
// Gauss-Newton leaves x; no positive-depth test in CheckInliers; pow(epsilon, 3).
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <cmath>

#include "../../include/vsg_orb.h"
#include "vsg_jacobi.h"
#include "vsg_math.h"
#include "vsg_pose_opt.h"

#if defined(__HIPCC__)
#define VSG_MLPNP_UNROLL _Pragma("unroll")
#define VSG_MLPNP_ROLLED _Pragma("unroll 1")
#else
#define VSG_MLPNP_UNROLL
#define VSG_MLPNP_ROLLED
#endif

namespace vsg {
namespace mlpnp {

// Jacobi sweeps: tests/test_mlpnp_reference.py measures the null vector against numpy.linalg.svd with these counts
enum { kSweeps = 12, kSweeps3 = 8 };
enum { kMaxHypotheses = 1024, kMinSet = 6, kGnRounds = 5 };
enum { kWork = 24 * 12 };  // doubles of the Jacobi's work matrix

struct Camera {
  float fx, fy, cx, cy;
};
// what the solver keeps of one correspondence: mvP2D, the bearing's x and y (z = 1), mvP3Dw, mvMaxError.  32 bytes
struct Point {
  float u, v, bx, by, X[3], max_err;
};
struct Pose {
  double R[9], t[3];  // row-major
};
// iterate's outcome: its return value, bNoMore, whether the pose is a Refine() return, the best hypothesis b (or -1), the
// hypothesis whose pose and flags are returned (or -1), mnIterations, how often the best set was replaced on the way
struct Selection {
  int found, no_more, refined, best, pose, iterations, records;
};

VSG_HD double canon(double v) { return v != v ? __builtin_nan("") : v; }
VSG_HD float canonf(float v) { return v != v ? __builtin_nanf("") : v; }
VSG_HD double dabs(double v) { return v < 0.0 ? -v : v; }

// the constructor's arithmetic for one correspondence: Pinhole::unproject (Pinhole.cpp:72-76) divided by its z = 1, and
// mvMaxError = sigma2 * th2 in float
VSG_HD Point make_point(const Camera &c, float u, float v, float sigma2, float th2, const float *X) {
  Point p;
  p.u = u, p.v = v;
  p.bx = fdiv(fsub(u, c.cx), c.fx), p.by = fdiv(fsub(v, c.cy), c.fy);
  p.X[0] = X[0], p.X[1] = X[1], p.X[2] = X[2];
  p.max_err = fmul(sigma2, th2);
  return p;
}

VSG_HD uint64_t d2u(double v) {
  union {
    double d;
    uint64_t u;
  } c;
  c.d = v;
  return c.u;
}
VSG_HD double u2d(uint64_t u) {
  union {
    double d;
    uint64_t u;
  } c;
  c.u = u;
  return c.d;
}

// ---- acos of a double: the fdlibm rational approximation, straight-line.  |x| > 1 or NaN: NaN.
VSG_HD double acos_ratio(double z) {
  const double pS0 = 1.66666666666666657415e-01, pS1 = -3.25565818622400915405e-01, pS2 = 2.01212532134862925881e-01,
               pS3 = -4.00555345006794114027e-02, pS4 = 7.91534994289814532176e-04, pS5 = 3.47933107596021167570e-05;
  const double qS1 = -2.40339491173441421878e+00, qS2 = 2.02094576023350569471e+00, qS3 = -6.88283971605453293030e-01,
               qS4 = 7.70381505559019352791e-02;
  const double p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
  const double q = 1.0 + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
  return p / q;
}
VSG_HD double dacos(double x) {
  const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17, pi = 3.14159265358979311600e+00;
  const double ax = dabs(x);
  if (!(ax <= 1.0)) return __builtin_nan("");
  if (ax == 1.0) return x > 0.0 ? 0.0 : pi + 2.0 * pio2_lo;
  if (ax < 0.5) {
    if (ax < 0x1p-57) return pio2_hi + pio2_lo;
    const double r = acos_ratio(x * x);
    return pio2_hi - (x - (pio2_lo - x * r));
  }
  if (x < 0.0) {
    const double z = (1.0 + x) * 0.5, s = dsqrt(z), r = acos_ratio(z), w = r * s - pio2_lo;
    return pi - 2.0 * (s + w);
  }
  const double z = (1.0 - x) * 0.5, s = dsqrt(z);
  const double df = u2d(d2u(s) & 0xffffffff00000000ull);
  const double c = (z - df * df) / (s + df), r = acos_ratio(z), w = r * s + c;
  return 2.0 * (df + w);
}

// ---- cube root of a double >= 0 (the solver takes it of an absolute value): exponent split by bits, a 5-bit start
// from the high word as fdlibm's cbrt has it, five Newton steps.  0 -> 0, inf -> inf, NaN -> NaN; negative: NaN.
VSG_HD double dcbrt(double x) {
  if (x != x || x < 0.0) return __builtin_nan("");
  if (x == 0.0 || x == __builtin_inf()) return x;
  double a = x, post = 1.0;
  if (a < 0x1p-1022) a = a * 0x1p54, post = 0x1p-18;  // subnormal: normalise
  const uint32_t hx = (uint32_t)(d2u(a) >> 32);
  double t = u2d((uint64_t)(hx / 3 + 715094163u) << 32);
  VSG_MLPNP_UNROLL
  for (int k = 0; k < 5; k++) t = t - (t - a / (t * t)) / 3.0;
  return t * post;
}

// CheckInliers' test of one correspondence (:275-299): the double pose times the float point, summed in double, stored
// to float; Pinhole::project in float; no positive-depth test
VSG_HD bool is_inlier(const Pose &T, const Camera &cam, const Point &p) {
  const double X = (double)p.X[0], Y = (double)p.X[1], Z = (double)p.X[2];
  const float xc = (float)(T.R[0] * X + T.R[1] * Y + T.R[2] * Z + T.t[0]);
  const float yc = (float)(T.R[3] * X + T.R[4] * Y + T.R[5] * Z + T.t[1]);
  const float zc = (float)(T.R[6] * X + T.R[7] * Y + T.R[8] * Z + T.t[2]);
  const float uu = fadd(fdiv(fmul(cam.fx, xc), zc), cam.cx), vv = fadd(fdiv(fmul(cam.fy, yc), zc), cam.cy);
  const float dx = fsub(p.u, uu), dy = fsub(p.v, vv);
  const float e2 = fadd(fmul(dx, dx), fmul(dy, dy));
  return e2 < p.max_err;
}

// the nullspace pair of the bearing (bx, by, 1) (deviation 1)
VSG_HD void nullspace(const Point &p, double *r, double *s) {
  const double x = (double)p.bx, y = (double)p.by;
  const double n = dsqrt(x * x + y * y + 1.0), z = 1.0 + n;
  const double uu = x * x + y * y + z * z, k = 2.0 / uu;
  r[0] = 1.0 - k * x * x, r[1] = -(k * x * y), r[2] = -(k * x * z);
  s[0] = -(k * y * x), s[1] = 1.0 - k * y * y, s[2] = -(k * y * z);
}

VSG_HD double sel3(const double *a, int i) { return i == 0 ? a[0] : i == 1 ? a[1] : a[2]; }
VSG_HD double det3(const double m[3][3]) {
  return m[0][0] * (m[1][1] * m[2][2] - m[1][2] * m[2][1]) - m[0][1] * (m[1][0] * m[2][2] - m[1][2] * m[2][0]) +
         m[0][2] * (m[1][0] * m[2][1] - m[1][1] * m[2][0]);
}

// rank of a 3 x 3 matrix as Eigen::FullPivHouseholderQR has it: full pivoting on the largest remaining entry, Householder
// reflections, the elimination stops at a remaining corner whose largest entry is <= 3 eps, and the rank counts the
// pivots above 3 eps times the largest pivot
VSG_HD int rank3(const double M[3][3]) {
  const double eps3 = 3.0 * 0x1p-52;
  double a[3][3];
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_MLPNP_UNROLL
    for (int j = 0; j < 3; j++) a[i][j] = M[i][j];
  double piv[3] = {0.0, 0.0, 0.0}, maxpiv = 0.0;
  bool live = true;
  VSG_MLPNP_UNROLL
  for (int k = 0; k < 3; k++) {
    double big = -1.0;
    int bi = k, bj = k;
    VSG_MLPNP_UNROLL
    for (int j = k; j < 3; j++)
      VSG_MLPNP_UNROLL
      for (int i = k; i < 3; i++) {
        const double v = dabs(a[i][j]);
        if (v > big) big = v, bi = i, bj = j;
      }
    if (!(big > eps3)) live = false;
    if (live) {
      VSG_MLPNP_UNROLL
      for (int j = 0; j < 3; j++) {  // rows k and bi, columns k and bj change places
        VSG_MLPNP_UNROLL
        for (int i = k; i < 3; i++)
          if (i == bi && i != k) {
            const double t = a[k][j];
            a[k][j] = a[i][j], a[i][j] = t;
          }
      }
      VSG_MLPNP_UNROLL
      for (int i = 0; i < 3; i++) {
        VSG_MLPNP_UNROLL
        for (int j = k; j < 3; j++)
          if (j == bj && j != k) {
            const double t = a[i][k];
            a[i][k] = a[i][j], a[i][j] = t;
          }
      }
      const double c0 = a[k][k];
      double tail = 0.0;
      VSG_MLPNP_UNROLL
      for (int i = k + 1; i < 3; i++) tail = tail + a[i][k] * a[i][k];
      double beta = c0, tau = 0.0, ess[3] = {0.0, 0.0, 0.0};
      if (tail > 0x1p-1022) {
        beta = dsqrt(c0 * c0 + tail);
        if (c0 >= 0.0) beta = -beta;
        VSG_MLPNP_UNROLL
        for (int i = k + 1; i < 3; i++) ess[i] = a[i][k] / (c0 - beta);
        tau = (beta - c0) / beta;
      }
      VSG_MLPNP_UNROLL
      for (int j = k + 1; j < 3; j++) {
        double tmp = a[k][j];
        VSG_MLPNP_UNROLL
        for (int i = k + 1; i < 3; i++) tmp = tmp + ess[i] * a[i][j];
        a[k][j] = a[k][j] - tau * tmp;
        VSG_MLPNP_UNROLL
        for (int i = k + 1; i < 3; i++) a[i][j] = a[i][j] - tau * ess[i] * tmp;
      }
      piv[k] = dabs(beta);
      if (piv[k] > maxpiv) maxpiv = piv[k];
    }
  }
  int rank = 0;
  VSG_MLPNP_UNROLL
  for (int k = 0; k < 3; k++) rank += piv[k] > maxpiv * eps3 ? 1 : 0;
  return rank;
}

// one-sided Jacobi of a 3 x 3 matrix in registers: US = U * Sigma, V
VSG_HD void svd3(const double T[3][3], double US[3][3], double V[3][3]) {
  JacobiRegs<3, 3> s;
  VSG_MLPNP_UNROLL
  for (int r = 0; r < 3; r++)
    VSG_MLPNP_UNROLL
    for (int c = 0; c < 3; c++) s.at(r, c) = T[r][c], s.at(3 + r, c) = r == c ? 1.0 : 0.0;
  jacobi_sweeps<3, 3, kSweeps3>(s);
  VSG_MLPNP_UNROLL
  for (int r = 0; r < 3; r++)
    VSG_MLPNP_UNROLL
    for (int c = 0; c < 3; c++) US[r][c] = s.at(r, c), V[r][c] = s.at(3 + r, c);
}
// U V^T of T's SVD (:567-568, :629-630); a zero singular value divides 0 by 0: NaN
VSG_HD void nearest_rotation(const double T[3][3], double R[3][3]) {
  double US[3][3], V[3][3];
  svd3(T, US, V);
  VSG_MLPNP_UNROLL
  for (int c = 0; c < 3; c++) {
    const double n = dsqrt(US[0][c] * US[0][c] + US[1][c] * US[1][c] + US[2][c] * US[2][c]);
    VSG_MLPNP_UNROLL
    for (int r = 0; r < 3; r++) US[r][c] = US[r][c] / n;
  }
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_MLPNP_UNROLL
    for (int j = 0; j < 3; j++) R[i][j] = US[i][0] * V[j][0] + US[i][1] * V[j][1] + US[i][2] * V[j][2];
}
// rows of E = the eigenvectors of the symmetric positive semi-definite M in ascending eigenvalue order (:406-408, deviation 2)
VSG_HD void eigen_rows_ascending(const double M[3][3], double E[3][3]) {
  double US[3][3], V[3][3], ev[3];
  svd3(M, US, V);
  VSG_MLPNP_UNROLL
  for (int c = 0; c < 3; c++) ev[c] = US[0][c] * US[0][c] + US[1][c] * US[1][c] + US[2][c] * US[2][c];
  VSG_MLPNP_UNROLL
  for (int c = 0; c < 3; c++) {
    int rank = 0;  // how many columns come before c
    VSG_MLPNP_UNROLL
    for (int o = 0; o < 3; o++) rank += (ev[o] < ev[c] || (ev[o] == ev[c] && o < c)) ? 1 : 0;
    double v[3] = {V[0][c], V[1][c], V[2][c]};
    double big = dabs(v[0]), lead = v[0];
    if (dabs(v[1]) > big) big = dabs(v[1]), lead = v[1];
    if (dabs(v[2]) > big) big = dabs(v[2]), lead = v[2];
    const bool neg = lead < 0.0;
    VSG_MLPNP_UNROLL
    for (int row = 0; row < 3; row++)
      if (row == rank) E[row][0] = neg ? -v[0] : v[0], E[row][1] = neg ? -v[1] : v[1], E[row][2] = neg ? -v[2] : v[2];
  }
}

// The Jacobi's work matrix in memory, 2 N rows of N doubles: thread `who` of `stride` rotates the rows who, who + stride,
// ...; sync() is the workgroup's barrier on the device (every thread of the workgroup runs the routine on identical
// bits), nothing on the host (who = 0, stride = 1)
template <int N>
struct JacobiMem {
  static constexpr bool kUnrolled = false;
  double *w;
  int who, stride;
  VSG_HD double &at(int r, int c) { return w[r * N + c]; }
  template <class F>
  VSG_HD void rows(F f) {
    for (int r = who; r < 2 * N; r += stride) f(r);
  }
  VSG_HD void sync() {
#if defined(__HIP_DEVICE_COMPILE__)
    __syncthreads();
#endif
  }
};

// rodrigues2rot (:685-700)
VSG_HD void rodrigues2rot(const double *w, double R[3][3]) {
  const double n2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], n = dsqrt(n2);
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_MLPNP_UNROLL
    for (int j = 0; j < 3; j++) R[i][j] = i == j ? 1.0 : 0.0;
  if (n > 0x1p-52) {
    double sn, cs;
    pose::sincos_pose(n, &sn, &cs);
    const double K[3][3] = {{0.0, -w[2], w[1]}, {w[2], 0.0, -w[0]}, {-w[1], w[0], 0.0}};
    const double a = sn / n, b = (1.0 - cs) / (n * n);
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_MLPNP_UNROLL
      for (int j = 0; j < 3; j++) {
        const double k2 = K[i][0] * K[0][j] + K[i][1] * K[1][j] + K[i][2] * K[2][j];
        R[i][j] = R[i][j] + a * K[i][j] + b * k2;
      }
  }
}
// rot2rodrigues (:702-718)
VSG_HD void rot2rodrigues(const double R[3][3], double *w) {
  w[0] = w[1] = w[2] = 0.0;
  const double trace = R[0][0] + R[1][1] + R[2][2] - 1.0;
  const double wnorm = dacos(trace / 2.0);
  if (wnorm > 0x1p-52) {
    double sn, cs;
    pose::sincos_pose(wnorm, &sn, &cs);
    const double sc = wnorm / (2.0 * sn);
    w[0] = (R[2][1] - R[1][2]) * sc, w[1] = (R[0][2] - R[2][0]) * sc, w[2] = (R[1][0] - R[0][1]) * sc;
  }
}

// what a Gauss-Newton round holds of x: R(w), w, t
struct GnState {
  double R[3][3], w[3], t[3], n2;
  bool at_zero;
};
VSG_HD GnState gn_state(const double *x) {
  GnState g;
  g.w[0] = x[0], g.w[1] = x[1], g.w[2] = x[2], g.t[0] = x[3], g.t[1] = x[4], g.t[2] = x[5];
  rodrigues2rot(g.w, g.R);
  g.n2 = x[0] * x[0] + x[1] * x[1] + x[2] * x[2];
  g.at_zero = !(dsqrt(g.n2) > 0x1p-52);
  return g;
}
VSG_HD void cross3(const double *a, const double *b, double *o) {
  o[0] = a[1] * b[2] - a[2] * b[1], o[1] = a[2] * b[0] - a[0] * b[2], o[2] = a[0] * b[1] - a[1] * b[0];
}
// residuals and Jacobian rows of one correspondence (:790-836 and deviation 6): res = n_{r,s}^T normalize(R X + t)
VSG_HD void gn_rows(const GnState &g, const Point &p, double *Jr, double *Js, double *res_r, double *res_s) {
  double nr[3], ns[3];
  nullspace(p, nr, ns);
  const double X[3] = {(double)p.X[0], (double)p.X[1], (double)p.X[2]};
  double Y[3], pc[3], v[3];
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++) Y[i] = g.R[i][0] * X[0] + g.R[i][1] * X[1] + g.R[i][2] * X[2], pc[i] = Y[i] + g.t[i];
  const double len = dsqrt(pc[0] * pc[0] + pc[1] * pc[1] + pc[2] * pc[2]);
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++) v[i] = pc[i] / len;
  *res_r = nr[0] * v[0] + nr[1] * v[1] + nr[2] * v[2], *res_s = ns[0] * v[0] + ns[1] * v[1] + ns[2] * v[2];
  // g_n = (n - v (v . n)) / |p|: the gradient of n^T normalize(p) by p
  double gr[3], gs[3];
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++) gr[i] = (nr[i] - v[i] * *res_r) / len, gs[i] = (ns[i] - v[i] * *res_s) / len;
  double wxY[3];
  cross3(g.w, Y, wxY);
  VSG_MLPNP_UNROLL
  for (int k = 0; k < 3; k++) {
    double d[3];  // d(R X) / dw_k
    double e[3] = {k == 0 ? 1.0 : 0.0, k == 1 ? 1.0 : 0.0, k == 2 ? 1.0 : 0.0};
    if (g.at_zero) {
      cross3(e, Y, d);
    } else {
      const double a[3] = {e[0] - g.R[0][k], e[1] - g.R[1][k], e[2] - g.R[2][k]};
      double b[3], bxY[3];
      cross3(g.w, a, b), cross3(b, Y, bxY);
      VSG_MLPNP_UNROLL
      for (int i = 0; i < 3; i++) d[i] = (g.w[k] * wxY[i] + bxY[i]) / g.n2;
    }
    Jr[k] = gr[0] * d[0] + gr[1] * d[1] + gr[2] * d[2], Js[k] = gs[0] * d[0] + gs[1] * d[1] + gs[2] * d[2];
    Jr[3 + k] = gr[k], Js[3 + k] = gs[k];
  }
}

// dx of A dx = g, A symmetric 6 x 6 (its upper triangle in `up`, row by row), LDL^T without pivoting (deviation 4)
VSG_HD void solve6(const double *up, const double *g, double *dx) {
  double A[6][6], L[6][6], d[6], y[6];
  int q = 0;
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 6; i++)
    VSG_MLPNP_UNROLL
    for (int j = i; j < 6; j++) A[i][j] = A[j][i] = up[q++];
  VSG_MLPNP_UNROLL
  for (int j = 0; j < 6; j++) {
    double s = A[j][j];
    VSG_MLPNP_UNROLL
    for (int k = 0; k < j; k++) s = s - L[j][k] * L[j][k] * d[k];
    d[j] = s;
    VSG_MLPNP_UNROLL
    for (int i = j + 1; i < 6; i++) {
      double t = A[i][j];
      VSG_MLPNP_UNROLL
      for (int k = 0; k < j; k++) t = t - L[i][k] * L[j][k] * d[k];
      L[i][j] = t / s;
    }
  }
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 6; i++) {
    double s = g[i];
    VSG_MLPNP_UNROLL
    for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
    y[i] = s;
  }
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 6; i++) y[i] = y[i] / d[i];
  VSG_MLPNP_UNROLL
  for (int i = 5; i >= 0; i--) {
    double s = y[i];
    VSG_MLPNP_UNROLL
    for (int k = i + 1; k < 6; k++) s = s - L[k][i] * dx[k];
    dx[i] = s;
  }
}

// mlpnp_gn (:720-788) on the Team's set; gn (may be nullptr): {rounds entered, 1 = aborted, max|dx|, min|dx|, max|J dx|}
// of the last round, for the tests
template <class Team>
VSG_HD void gauss_newton(Team &tm, double *x, double *gn) {
  VSG_MLPNP_ROLLED
  for (int it = 0; it < kGnRounds; it++) {
    const GnState g = gn_state(x);
    double acc[27], dx[6];
    tm.template sum<27>(
        [&](const Point &p, double *o) {
          double Jr[6], Js[6], rr, rs;
          gn_rows(g, p, Jr, Js, &rr, &rs);
          int q = 0;
          VSG_MLPNP_UNROLL
          for (int a = 0; a < 6; a++)
            VSG_MLPNP_UNROLL
            for (int b = a; b < 6; b++) o[q++] = Jr[a] * Jr[b] + Js[a] * Js[b];
          VSG_MLPNP_UNROLL
          for (int a = 0; a < 6; a++) o[21 + a] = Jr[a] * rr + Js[a] * rs;
        },
        acc);
    solve6(acc, acc + 21, dx);
    double amax = dabs(dx[0]), amin = dabs(dx[0]);  // maxCoeff / minCoeff: entry 0, then strict comparisons
    VSG_MLPNP_UNROLL
    for (int k = 1; k < 6; k++) {
      const double a = dabs(dx[k]);
      if (a > amax) amax = a;
      if (a < amin) amin = a;
    }
    if (gn) gn[0] = (double)(it + 1), gn[1] = 0.0, gn[2] = amax, gn[3] = amin, gn[4] = 0.0;
    if (amax > 5.0 || amin > 1.0) {  // :772: x stays as it was
      if (gn) gn[1] = 1.0;
      break;
    }
    const double dl = tm.max0([&](const Point &p) {
      double Jr[6], Js[6], rr, rs;
      gn_rows(g, p, Jr, Js, &rr, &rs);
      double a = 0.0, b = 0.0;
      VSG_MLPNP_UNROLL
      for (int k = 0; k < 6; k++) a = a + Jr[k] * dx[k], b = b + Js[k] * dx[k];
      a = dabs(a), b = dabs(b);
      return b > a ? b : a;
    });
    if (gn) gn[4] = dl;
    VSG_MLPNP_UNROLL
    for (int k = 0; k < 6; k++) x[k] = x[k] - dx[k];
    if (dl < 1e-5) break;  // :776: the step is applied first
  }
}

// entry j of the design matrix's two rows of one correspondence (:455-533): NC = 12 or 9 columns, P = the (rotated) point
template <int NC>
VSG_HD void design_entry(const double *r, const double *s, const double *P, int j, double *er, double *es) {
  if (NC == 12) {
    if (j < 9) {
      const double c = sel3(P, j % 3);
      *er = sel3(r, j / 3) * c, *es = sel3(s, j / 3) * c;
    } else {
      *er = sel3(r, j - 9), *es = sel3(s, j - 9);
    }
  } else {
    if (j < 6) {
      const double c = (j & 1) ? P[2] : P[1];
      *er = sel3(r, j >> 1) * c, *es = sel3(s, j >> 1) * c;
    } else {
      *er = sel3(r, j - 6), *es = sel3(s, j - 6);
    }
  }
}
// A^T A of the set into the work matrix, the Jacobi, the null vector (:538-545, deviations 2 and 3).  E: eigenRot
template <int NC, class Team>
VSG_HD void null_vector(Team &tm, double *work, int who, int stride, const double E[3][3], double *v) {
  JacobiMem<NC> s = {work, who, stride};
  s.sync();  // whoever still reads the matrix of the solve before has finished
  VSG_MLPNP_ROLLED
  for (int j = 0; j < NC; j++) {
    double acc[NC];
    tm.template sum<NC>(
        [&](const Point &p, double *o) {
          double r[3], q[3], P[3];
          nullspace(p, r, q);
          const double X[3] = {(double)p.X[0], (double)p.X[1], (double)p.X[2]};
          VSG_MLPNP_UNROLL
          for (int i = 0; i < 3; i++) P[i] = E[i][0] * X[0] + E[i][1] * X[1] + E[i][2] * X[2];
          double jr, js;
          design_entry<NC>(r, q, P, j, &jr, &js);
          VSG_MLPNP_UNROLL
          for (int k = 0; k < NC; k++) {
            double kr, ks;
            design_entry<NC>(r, q, P, k, &kr, &ks);
            o[k] = jr * kr + js * ks;
          }
        },
        acc);
    if (who == 0) {
      VSG_MLPNP_UNROLL
      for (int k = 0; k < NC; k++) s.at(j, k) = acc[k];
    }
  }
  s.rows([&](int r) {
    if (r >= NC) jacobi_identity_row<NC, NC>(s, r);
  });
  s.sync();
  jacobi_sweeps<NC, NC, kSweeps>(s);
  jacobi_null_vector<NC, NC>(s, v);
}

// computePose (:365-683) on the Team's set.  work: kWork doubles that every thread of the Team's workgroup sees (LDS on the
// device); who / stride: this thread among those that run the routine side by side on identical bits.  info (may be
// nullptr): {planar, err0, err1 (the direction test's two smallest candidates), gn[5]} for the tests.
template <class Team>
VSG_HD void compute_pose(Team &tm, double *work, int who, int stride, Pose *out, double *info) {
  // 1. planar?  (:392-411)
  double m6[6];
  tm.template sum<6>(
      [&](const Point &p, double *o) {
        const double x = (double)p.X[0], y = (double)p.X[1], z = (double)p.X[2];
        o[0] = x * x, o[1] = x * y, o[2] = x * z, o[3] = y * y, o[4] = y * z, o[5] = z * z;
      },
      m6);
  const double M[3][3] = {{m6[0], m6[1], m6[2]}, {m6[1], m6[3], m6[4]}, {m6[2], m6[4], m6[5]}};
  const bool planar = rank3(M) == 2;
  double E[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};  // eigenRot
  if (planar) eigen_rows_ascending(M, E);
  // 3, 4. the design matrix's normal equations and their null vector
  double v[12];
  VSG_MLPNP_UNROLL
  for (int k = 0; k < 12; k++) v[k] = 0.0;
  if (planar) {
    null_vector<9>(tm, work, who, stride, E, v);
  } else {
    const double I3[3][3] = {{1.0, 0.0, 0.0}, {0.0, 1.0, 0.0}, {0.0, 0.0, 1.0}};
    null_vector<12>(tm, work, who, stride, I3, v);
  }
  double T[3][3], scale;
  if (planar) {  // :555-565: rows (col1 x col2), (v0 v2 v4), (v1 v3 v5) after the transposition
    const double c1[3] = {v[0], v[2], v[4]}, c2[3] = {v[1], v[3], v[5]};
    double c0[3];
    cross3(c1, c2, c0);
    VSG_MLPNP_UNROLL
    for (int j = 0; j < 3; j++) T[0][j] = c0[j], T[1][j] = c1[j], T[2][j] = c2[j];
    const double n1 = dsqrt(T[0][1] * T[0][1] + T[1][1] * T[1][1] + T[2][1] * T[2][1]);
    const double n2 = dsqrt(T[0][2] * T[0][2] + T[1][2] * T[1][2] + T[2][2] * T[2][2]);
    scale = 1.0 / dsqrt(dabs(n1 * n2));
  } else {  // :620-626
    VSG_MLPNP_UNROLL
    for (int r = 0; r < 3; r++)
      VSG_MLPNP_UNROLL
      for (int c = 0; c < 3; c++) T[r][c] = v[3 * c + r];
    double n[3];
    VSG_MLPNP_UNROLL
    for (int c = 0; c < 3; c++) n[c] = dsqrt(T[0][c] * T[0][c] + T[1][c] * T[1][c] + T[2][c] * T[2][c]);
    scale = 1.0 / dcbrt(dabs(n[0] * n[1] * n[2]));
  }
  double R0[3][3];
  nearest_rotation(T, R0);
  if (det3(R0) < 0) {
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_MLPNP_UNROLL
      for (int j = 0; j < 3; j++) R0[i][j] = -R0[i][j];
  }
  // the candidates of the direction test: nc of them, {R (one of two), t}
  double RA[3][3], RB[3][3], tc[4][3];
  int nc;
  if (planar) {  // :573-597
    double R1[3][3];
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_MLPNP_UNROLL
      for (int j = 0; j < 3; j++) R1[i][j] = E[0][i] * R0[0][j] + E[1][i] * R0[1][j] + E[2][i] * R0[2][j];  // eigenRot^T * Rout1
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_MLPNP_UNROLL
      for (int j = 0; j < 3; j++) RA[i][j] = -R1[j][i];  // transposeInPlace, *= -1
    if (det3(RA) < 0.0) RA[0][2] = -RA[0][2], RA[1][2] = -RA[1][2], RA[2][2] = -RA[2][2];
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++) RB[i][0] = -RA[i][0], RB[i][1] = -RA[i][1], RB[i][2] = RA[i][2];
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++) {
      const double t = scale * v[6 + i];
      tc[0][i] = t, tc[1][i] = -t, tc[2][i] = t, tc[3][i] = -t;
    }
    nc = 4;
  } else {  // :635-649: tout = Rout * (scale * t); the candidates are the inverses of [Rout | +-tout]
    const double ts[3] = {scale * v[9], scale * v[10], scale * v[11]};
    double tout[3];
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++) tout[i] = R0[i][0] * ts[0] + R0[i][1] * ts[1] + R0[i][2] * ts[2];
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++)
      VSG_MLPNP_UNROLL
      for (int j = 0; j < 3; j++) RA[i][j] = RB[i][j] = R0[j][i];
    VSG_MLPNP_UNROLL
    for (int i = 0; i < 3; i++) {
      const double t = -(RA[i][0] * tout[0] + RA[i][1] * tout[1] + RA[i][2] * tout[2]);
      tc[0][i] = t, tc[1][i] = -t, tc[2][i] = tc[3][i] = 0.0;
    }
    nc = 2;
  }
  // :599-616, :650-660 over the FIRST SIX correspondences of the set: sum of 1 - normalize(R X + t) . f
  double err[4] = {0.0, 0.0, 0.0, 0.0};
  VSG_MLPNP_UNROLL
  for (int c = 0; c < 4; c++) {
    if (c < nc) {
      VSG_MLPNP_ROLLED
      for (int q = 0; q < 6; q++) {
        const Point &p = tm.six(q);
        const double X[3] = {(double)p.X[0], (double)p.X[1], (double)p.X[2]};
        double y[3];
        VSG_MLPNP_UNROLL
        for (int i = 0; i < 3; i++) {
          const double a = c < 2 ? RA[i][0] : RB[i][0], b = c < 2 ? RA[i][1] : RB[i][1], d = c < 2 ? RA[i][2] : RB[i][2];
          y[i] = a * X[0] + b * X[1] + d * X[2] + tc[c][i];
        }
        const double len = dsqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
        const double dot = y[0] / len * (double)p.bx + y[1] / len * (double)p.by + y[2] / len;
        err[c] = err[c] + (1.0 - dot);
      }
    }
  }
  int pick = 0;
  if (planar) {  // min_element: the first of equal minima
    VSG_MLPNP_UNROLL
    for (int c = 1; c < 4; c++)
      if (err[c] < err[pick]) pick = c;
  } else {
    pick = err[0] < err[1] ? 0 : 1;
  }
  double Rout[3][3], x[6];
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++) {
    VSG_MLPNP_UNROLL
    for (int j = 0; j < 3; j++) Rout[i][j] = pick < 2 ? RA[i][j] : RB[i][j];
    x[3 + i] = pick == 0 ? tc[0][i] : pick == 1 ? tc[1][i] : pick == 2 ? tc[2][i] : tc[3][i];
  }
  // 5. Gauss-Newton (:667-682)
  rot2rodrigues(Rout, x);
  if (info) {
    double lo = err[0], hi = err[1];  // the chosen candidate and its closest rival decide the branch
    if (planar) {
      lo = err[pick], hi = __builtin_inf();
      for (int c = 0; c < 4; c++)
        if (c != pick && err[c] < hi) hi = err[c];
    }
    info[0] = planar ? 1.0 : 0.0, info[1] = lo, info[2] = hi;
  }
  gauss_newton(tm, x, info ? info + 3 : nullptr);
  double Rf[3][3];
  rodrigues2rot(x, Rf);
  VSG_MLPNP_UNROLL
  for (int i = 0; i < 3; i++) {
    VSG_MLPNP_UNROLL
    for (int j = 0; j < 3; j++) out->R[3 * i + j] = Rf[i][j];
    out->t[i] = x[3 + i];
  }
}

// the six samples of a hypothesis, summed serially in drawing order by whoever runs the hypothesis
struct SerialTeam {
  const Point *pts;
  const int32_t *set;
  template <int W, class F>
  VSG_HD void sum(F f, double *acc) {
    VSG_MLPNP_UNROLL
    for (int k = 0; k < W; k++) acc[k] = 0.0;
    VSG_MLPNP_ROLLED
    for (int j = 0; j < kMinSet; j++) {
      double o[W];
      f(pts[set[j]], o);
      VSG_MLPNP_UNROLL
      for (int k = 0; k < W; k++) acc[k] = acc[k] + o[k];
    }
  }
  template <class F>
  VSG_HD double max0(F f) {
    double m = 0.0;
    VSG_MLPNP_ROLLED
    for (int j = 0; j < kMinSet; j++) {
      const double v = f(pts[set[j]]);
      if (v > m) m = v;
    }
    return m;
  }
  VSG_HD const Point &six(int q) const { return pts[set[q]]; }
};

// iterate's loop (:120-228) entered at mnIterations == first, from the counts c[0 .. n_hyp).  The members before `first` are
// what the calls before left: every hypothesis walked updates the best.  end = max(max_its, first + n_iterations) <= n_hyp:
// the caller checked.
VSG_HD Selection select(const int32_t *c, int first, int n_iterations, int max_its, int min_inliers) {
  Selection s = {0, 0, 0, -1, -1, first, 0};
  const int walk = first + n_iterations, end = max_its > walk ? max_its : walk;
  int best_count = 0;
  for (int k = 0; k < end; k++) {
    const int ck = c[k];
    if (ck >= min_inliers) {                                          // :176, not strict
      if (ck > best_count) best_count = ck, s.best = k, s.records++;  // :179, strict: the first maximum stays
      if (k >= first && ck > min_inliers) {  // Refine() (:196): CheckInliers on hypothesis k's pose again, strict (:345)
        s.found = 1, s.refined = 1, s.pose = k, s.iterations = k + 1;
        return s;
      }
    }
  }
  if (end > first) s.iterations = end;
  if (s.iterations >= max_its) {  // :211-226: the best hypothesis as it is
    s.no_more = 1;
    if (s.best >= 0) s.found = 1, s.pose = s.best;
  }
  return s;
}

VSG_HD void fill_result(const Selection &s, const Pose *T /* nullptr: the identity */, int n_inliers, int n, vsg_mlpnp_result *res) {
  for (int i = 0; i < 16; i++) res->Tcw[i] = i % 5 == 0 ? 1.0f : 0.0f;
  if (T) {
    for (int i = 0; i < 3; i++) {
      for (int j = 0; j < 3; j++) res->Tcw[4 * i + j] = canonf((float)T->R[3 * i + j]);
      res->Tcw[4 * i + 3] = canonf((float)T->t[i]);
    }
  }
  res->found = s.found, res->no_more = s.no_more, res->n_inliers = n_inliers, res->refined = s.refined;
  res->best_hypothesis = s.best, res->iterations = s.iterations, res->n_correspondences = n, res->n_records = s.records;
}
// N < mRansacMinInliers (:111-115)
inline void fill_no_more(int n, vsg_mlpnp_result *res) {
  const Selection s = {0, 1, 0, -1, -1, 0, 0};
  fill_result(s, nullptr, 0, n, res);
}

// ---- the host's side of a call

// the members of a set among n correspondences, summed in index order (host only)
struct MemberTeam {
  const Point *pts;
  const uint8_t *member;
  int n;
  int first_six[6];
  void find_six() {
    int q = 0;
    for (int i = 0; i < n && q < 6; i++)
      if (member[i]) first_six[q++] = i;
    for (; q < 6; q++) first_six[q] = 0;  // fewer than six members: never, a best set has min_inliers >= 6 of them
  }
  template <int W, class F>
  void sum(F f, double *acc) {
    for (int k = 0; k < W; k++) acc[k] = 0.0;
    for (int i = 0; i < n; i++) {
      if (!member[i]) continue;
      double o[W];
      f(pts[i], o);
      for (int k = 0; k < W; k++) acc[k] = acc[k] + o[k];
    }
  }
  template <class F>
  double max0(F f) {
    double m = 0.0;
    for (int i = 0; i < n; i++) {
      if (!member[i]) continue;
      const double v = f(pts[i]);
      if (v > m) m = v;
    }
    return m;
  }
  const Point &six(int q) const { return pts[first_six[q]]; }
};

// what vsg_frame_mlpnp_ransac refuses before it enqueues, the handles and devices aside.  octave(i): the octave of feature
// i, asked only for features with a slot.  *n_out = the number of correspondences.
template <class OctaveOf>
inline bool args_ok(int n_feat, const int32_t *slots, int capacity, const float *level_sigma2, int nlevels, OctaveOf octave,
                    float th2, int min_inliers, int max_its, int first, int n_iterations, int n_hyp, const int32_t *sets,
                    const uint8_t *inlier, const vsg_mlpnp_result *res, int *n_out) {
  if (n_feat < 0 || !slots || !level_sigma2 || !sets || !inlier || !res) return false;
  if (nlevels < 1 || nlevels > 16 || !(th2 > 0.0f) || !(th2 < __builtin_inff())) return false;
  if (min_inliers < kMinSet || max_its < 1 || first < 0 || n_iterations < 0 || n_hyp < 1 || n_hyp > kMaxHypotheses) return false;
  if ((long long)first + n_iterations > n_hyp || max_its > n_hyp) return false;
  int n = 0;
  for (int i = 0; i < n_feat; i++) {
    if (slots[i] < 0) continue;
    if (slots[i] >= capacity) return false;
    const int o = octave(i);
    if (o < 0 || o >= nlevels) return false;
    n++;
  }
  *n_out = n;
  if (n < min_inliers) return true;  // nothing is computed: the sets are not read
  for (int k = 0; k < n_hyp; k++) {
    const int32_t *s = sets + 6 * (size_t)k;
    for (int a = 0; a < 6; a++) {
      if (s[a] < 0 || s[a] >= n) return false;
      for (int b = 0; b < a; b++)
        if (s[a] == s[b]) return false;
    }
  }
  return true;
}

struct HostWork {
  double w[kWork];
};

// one hypothesis on the host
inline void hypothesis_host(const Point *pts, const int32_t *set, Pose *T, double *info) {
  HostWork wk;
  SerialTeam tm = {pts, set};
  compute_pose(tm, wk.w, 0, 1, T, info);
}
// computePose over the set `member`: the solve Refine() runs over the best set (:305-337) and discards
inline void member_pose_host(const Point *pts, const uint8_t *member, int n, Pose *T, double *info) {
  HostWork wk;
  MemberTeam tm = {pts, member, n, {0, 0, 0, 0, 0, 0}};
  tm.find_six();
  compute_pose(tm, wk.w, 0, 1, T, info);
}
VSG_HD void canon_pose(const Pose &T, double *o) {
  for (int i = 0; i < 3; i++) {
    for (int j = 0; j < 3; j++) o[4 * i + j] = canon(T.R[3 * i + j]);
    o[4 * i + 3] = canon(T.t[i]);
  }
}

// vsg_frame_mlpnp_ransac on arrays the caller holds: per feature the keypoint, its octave and, where slots[i] >= 0, the
// position world_pos[3 * slots[i]].  The arguments have passed args_ok (n = its count).  Every hypothesis is computed, as
// on the device.
inline void ransac_host(int n_feat, const int32_t *slots, const float *world_pos, const float *kx, const float *ky,
                        const int32_t *octave, const Camera &cam, const float *level_sigma2, float th2, int min_inliers,
                        int max_its, int first, int n_iterations, int n_hyp, const int32_t *sets, int n, Point *pts /* n */,
                        uint8_t *inlier, vsg_mlpnp_result *res, int32_t *hyp_inliers, double *hyp_T) {
  for (int i = 0; i < n_feat; i++) inlier[i] = 0;
  if (n < min_inliers) {
    fill_no_more(n, res);
    return;
  }
  for (int i = 0, e = 0; i < n_feat; i++)
    if (slots[i] >= 0) pts[e++] = make_point(cam, kx[i], ky[i], level_sigma2[octave[i]], th2, world_pos + 3 * (size_t)slots[i]);
  static thread_local int32_t counts[kMaxHypotheses];
  static thread_local Pose hyp[kMaxHypotheses];
  for (int k = 0; k < n_hyp; k++) {
    hypothesis_host(pts, sets + 6 * (size_t)k, &hyp[k], nullptr);
    int c = 0;
    for (int i = 0; i < n; i++) c += is_inlier(hyp[k], cam, pts[i]) ? 1 : 0;
    counts[k] = c;
    if (hyp_inliers) hyp_inliers[k] = c;
    if (hyp_T) canon_pose(hyp[k], hyp_T + 12 * (size_t)k);
  }
  const Selection s = select(counts, first, n_iterations, max_its, min_inliers);
  const Pose *T = s.pose >= 0 ? &hyp[s.pose] : nullptr;
  if (T)
    for (int i = 0, e = 0; i < n_feat; i++)
      if (slots[i] >= 0) inlier[i] = is_inlier(*T, cam, pts[e++]) ? 1 : 0;
  fill_result(s, T, T ? counts[s.pose] : 0, n, res);
}

// SetRansacParameters (:231-262) as written
inline int cvt_int_x86_d(double v) { return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (int)0x80000000; }
inline void ransac_parameters(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, int n,
                              int *min_inliers_out, int *max_its_out) {
  int nMinInliers = cvt_int_x86((float)n * epsilon);  // int = int * float
  if (nMinInliers < min_inliers) nMinInliers = min_inliers;
  if (nMinInliers < min_set) nMinInliers = min_set;
  if (epsilon < (float)nMinInliers / n) epsilon = (float)nMinInliers / n;
  int nIterations;
  if (nMinInliers == n)
    nIterations = 1;
  else  // pow(float, int) promotes to double
    nIterations = cvt_int_x86_d(std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3))));
  const int capped = nIterations < max_iterations ? nIterations : max_iterations;
  *min_inliers_out = nMinInliers, *max_its_out = capped > 1 ? capped : 1;
}

}  // namespace mlpnp
}  // namespace vsg
