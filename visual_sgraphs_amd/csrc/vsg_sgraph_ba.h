// vsg_sgraph_ba.h -- the planes and rooms of Optimizer::LocalBundleAdjustment (Optimizer.cc:2018-2232, :2342-2369,
// :2426-2441) behind the visual part of vsg_local_ba.h, host and device from one source.  The kernels of vsg_sgraph_ba.hip
// run the per-item functions below; tests/_sgbacore and the latency probe's caller-side loop compile the same functions for
// the host and replay every sum in the same tree (HostRun).
//
// Everything is double, as g2o has it.  What is restated, and from where:
//   * g2o::Plane3D (Thirdparty/g2o/g2o/types/plane3d.h): normalize (:101), operator*(Isometry3D, Plane3D) (:108), azimuth
//     (:57), elevation (:59), rotation (:64: AngleAxis(az, Z) * AngleAxis(-el, Y) is a product of two quaternions turned
//     into a matrix), oplus (:73), ominus (:89).  VertexPlane has dimension 3; setEstimate copies and does not renormalise;
//   * atan2 as fdlibm has it (e_atan2.c, s_atan.c), written out straight-line; sin / cos are vsg_pose_opt.h's, extended to
//     negative arguments by symmetry;
//   * EdgeSE3KFPointToPlane (OptimizableTypes.h:296), EdgeVertexPlaneProjectSE3KF (:336), EdgeVertex2PlaneProjectSE3Room
//     (:452) and EdgeVertex4PlaneProjectSE3Room (:508): computeError, correctPlaneDirection, isDistanceCorrect, their
//     informations (Optimizer.cc:2090, :2115, :2188, :2207) and the float Huber deltas of :1846-1848;
//   * the numeric Jacobians of base_binary_edge.hpp:131-202 and base_multi_edge.hpp:63-126 (delta = 1e-9, central
//     difference, scalar * errorBak, fixed vertices skipped) and constructQuadraticForm of both bases with the robust
//     kernel (base_binary_edge.hpp:91-113, base_multi_edge.hpp:171-222 under robustInformation(rho), omega_r * rho[1]);
//   * the classification (:2342-2369) with chi2 as the LAST computeActiveErrors left it and isDistanceCorrect on the
//     restored estimates, and the recovery (:2427-2441).
//
// THE SYSTEM.  The planes and rooms are not marginalised, so they are rows of the reduced system behind the optimised
// keyframes: the planes that have an edge (3 rows each, list order), then the rooms (6 rows each: VertexSE3Expmap, although
// the error reads the translation alone).  None of these edges touches a map point, so the Schur complement over the
// points is the visual call's, written into the larger matrix (lba::Prob::n is the row stride).  lambda goes on the new
// diagonals, and lba::begin_iteration / lba::decide see the new vertices and edges as further partials behind the visual
// ones (chiPart, maxPart, scalePart), a keyframe's semantic blocks inside its Hpp / bp.
//
// ORDERS.  Semantic edges: per plane, per observation, the plane-keyframe edge before the point-to-plane edge; then the
// rooms.  Every sum is one fixed tree:
//   * an edge's blocks: serial over the error's rows;
//   * a keyframe's Hpp / bp: the visual tree's result, then its semantic edges serially in edge order;
//   * a semantic row's b and diagonal, and every entry of a block of the system: serial over the contributing edges;
//   * the robust chi2 of the semantic edges, the lambda-init maximum and computeScale over the semantic rows: groups of
//     kThreads through lba's tree, the partials serially behind the visual ones.
// No floating-point atomics.  Both builds use -ffp-contract=off.  Every loop bound is a constant or a count the host validated.
#pragma once
#include "vsg_local_ba.h"
#include "vsg_mlpnp.h"

#if defined(__HIPCC__)
#define VSG_SGBA_UNROLL _Pragma("unroll")
#else
#define VSG_SGBA_UNROLL
#endif

namespace vsg {
namespace sgba {

enum { kPointPlane = 0, kPlaneKf = 1, kRoom2 = 2, kRoom4 = 3 };  // edge kinds
enum { kMaxCols = 18, kMaxSlots = 2 * kMaxCols + 1, kMaxRows = 6 * lba::kMaxOptKf, oB = kMaxCols * kMaxCols, kBlock = oB + kMaxCols };
enum { kEdgesPerGroup = lba::kThreads / pose::kWave, kBlocksPerGroup = lba::kThreads / 36 };

using pose::Est;

// ---- atan and atan2: fdlibm's s_atan.c / e_atan2.c.  The tables are selects: no array is indexed by a variable.
VSG_HD double datan(double x) {
  const double aT0 = 3.33333333333329318027e-01, aT1 = -1.99999999998764832476e-01, aT2 = 1.42857142725034663711e-01,
               aT3 = -1.11111104054623557880e-01, aT4 = 9.09088713343650656196e-02, aT5 = -7.69187620504482999495e-02,
               aT6 = 6.66107313738753120669e-02, aT7 = -5.83357013379057348645e-02, aT8 = 4.97687799461593236017e-02,
               aT9 = -3.65315727442169155270e-02, aT10 = 1.62858201153657823623e-02;
  const uint32_t hx = (uint32_t)(mlpnp::d2u(x) >> 32), ix = hx & 0x7fffffffu;
  const bool neg = (hx >> 31) != 0;
  if (ix >= 0x44100000u) {  // |x| >= 2^66, inf, NaN
    if (x != x) return x + x;
    const double r = 1.57079632679489655800e+00 + 6.12323399573676603587e-17;
    return neg ? -r : r;
  }
  int id = -1;
  if (ix < 0x3fdc0000u) {  // |x| < 0.4375
    if (ix < 0x3e200000u) return x;
  } else {
    x = __builtin_fabs(x);
    if (ix < 0x3ff30000u) {
      if (ix < 0x3fe60000u)
        id = 0, x = (2.0 * x - 1.0) / (2.0 + x);
      else
        id = 1, x = (x - 1.0) / (x + 1.0);
    } else if (ix < 0x40038000u) {
      id = 2, x = (x - 1.5) / (1.0 + 1.5 * x);
    } else {
      id = 3, x = -1.0 / x;
    }
  }
  const double z = x * x, w = z * z;
  const double s1 = z * (aT0 + w * (aT2 + w * (aT4 + w * (aT6 + w * (aT8 + w * aT10)))));
  const double s2 = w * (aT1 + w * (aT3 + w * (aT5 + w * (aT7 + w * aT9))));
  if (id < 0) return x - x * (s1 + s2);
  const double hi = id == 0 ? 4.63647609000806093515e-01 : id == 1 ? 7.85398163397448278999e-01 : id == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
  const double lo = id == 0 ? 2.26987774529616870924e-17 : id == 1 ? 3.06161699786838301793e-17 : id == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
  const double r = hi - ((x * (s1 + s2) - lo) - x);
  return neg ? -r : r;
}
VSG_HD double datan2(double y, double x) {
  const double pi_o_4 = 7.8539816339744827900E-01, pi_o_2 = 1.5707963267948965580E+00, pi = 3.1415926535897931160E+00,
               pi_lo = 1.2246467991473531772E-16;
  if (x != x || y != y) return x + y;
  const uint64_t bx = mlpnp::d2u(x), by = mlpnp::d2u(y);
  const int32_t hx = (int32_t)(bx >> 32), hy = (int32_t)(by >> 32), ix = hx & 0x7fffffff, iy = hy & 0x7fffffff;
  const uint32_t lx = (uint32_t)bx, ly = (uint32_t)by;
  if (hx == 0x3ff00000 && lx == 0) return datan(y);  // x == 1
  const int m = ((hy >> 31) & 1) | ((hx >> 30) & 2);  // 2 * sign(x) + sign(y)
  if (iy == 0 && ly == 0) return m < 2 ? y : m == 2 ? pi : -pi;
  if (ix == 0 && lx == 0) return hy < 0 ? -pi_o_2 : pi_o_2;
  if (ix == 0x7ff00000) {
    if (iy == 0x7ff00000) return m == 0 ? pi_o_4 : m == 1 ? -pi_o_4 : m == 2 ? 3.0 * pi_o_4 : -3.0 * pi_o_4;
    return m == 0 ? 0.0 : m == 1 ? -0.0 : m == 2 ? pi : -pi;
  }
  if (iy == 0x7ff00000) return hy < 0 ? -pi_o_2 : pi_o_2;
  const int32_t k = (iy - ix) >> 20;
  double z;
  if (k > 60)
    z = pi_o_2 + 0.5 * pi_lo;  // |y / x| > 2^60
  else if (hx < 0 && k < -60)
    z = 0.0;  // |y| / x < -2^60
  else
    z = datan(__builtin_fabs(y / x));
  return m == 0 ? z : m == 1 ? -z : m == 2 ? pi - (z - pi_lo) : (z - pi_lo) - pi;
}
// sin and cos of any sign: sin is odd, cos is even (beyond 1e5 or NaN both are NaN, as pose::sincos_pose has it)
VSG_HD void dsincos(double x, double *s, double *c) {
  pose::sincos_pose(__builtin_fabs(x), s, c);
  if (x < 0.0) *s = -*s;
}

// ---- g2o::Plane3D on four coefficients
VSG_HD void plane_normalize(double *c) {
  const double n = dsqrt((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]), inv = 1. / n;
  VSG_SGBA_UNROLL
  for (int k = 0; k < 4; k++) c[k] = c[k] * inv;
}
VSG_HD double azimuth(const double *v) { return datan2(v[1], v[0]); }
VSG_HD double elevation(const double *v) { return datan2(v[2], dsqrt(v[0] * v[0] + v[1] * v[1])); }
// (AngleAxis(az, UnitZ) * AngleAxis(-el, UnitY)).toRotationMatrix(): Eigen multiplies the two as quaternions
VSG_HD void plane_rotation(const double *v, double R[3][3]) {
  const double az = azimuth(v), el = elevation(v);
  double sz, cz, sy, cy;
  dsincos(0.5 * az, &sz, &cz);
  dsincos(0.5 * -el, &sy, &cy);
  const double qz[4] = {sz * 0.0, sz * 0.0, sz * 1.0, cz}, qy[4] = {sy * 0.0, sy * 1.0, sy * 0.0, cy};
  double q[4];
  pose::quat_mul(qz, qy, q);
  lba::quat_to_matrix(q, R);
}
VSG_HD void plane_oplus(const double *c, const double *v, double *o) {
  double s, cc, sa, ca, R[3][3];
  dsincos(v[1], &s, &cc);
  dsincos(v[0], &sa, &ca);
  const double n[3] = {cc * ca, cc * sa, s};
  plane_rotation(c, R);
  const double d = -c[3] + v[2];
  VSG_SGBA_UNROLL
  for (int i = 0; i < 3; i++) o[i] = (R[i][0] * n[0] + R[i][1] * n[1]) + R[i][2] * n[2];
  o[3] = -d;
  plane_normalize(o);
}
// a.ominus(b)
VSG_HD void plane_ominus(const double *a, const double *b, double *e) {
  double R[3][3], n[3];
  plane_rotation(a, R);
  VSG_SGBA_UNROLL
  for (int i = 0; i < 3; i++) n[i] = (R[0][i] * b[0] + R[1][i] * b[1]) + R[2][i] * b[2];
  e[0] = azimuth(n), e[1] = elevation(n), e[2] = -a[3] - -b[3];
}
// Eigen::Isometry3d(SE3Quat) * Plane3D, normalised by the constructor
VSG_HD void plane_transform(const Est &T, const double *c, double *o) {
  double R[3][3];
  lba::quat_to_matrix(T.q, R);
  VSG_SGBA_UNROLL
  for (int i = 0; i < 3; i++) o[i] = (R[i][0] * c[0] + R[i][1] * c[1]) + R[i][2] * c[2];
  o[3] = c[3] - ((T.t[0] * o[0] + T.t[1] * o[1]) + T.t[2] * o[2]);
  plane_normalize(o);
}

// ---- the edges' computeError
// EdgeSE3KFPointToPlane: Pj^T Ti Gij Ti^T Pj, Ti = estimate().inverse().to_homogeneous_matrix(), left to right
VSG_HD double point_plane_error(const Est &T, const double *Pj, const double *G) {
  const double qi[4] = {-T.q[0], -T.q[1], -T.q[2], T.q[3]}, nt[3] = {T.t[0] * -1., T.t[1] * -1., T.t[2] * -1.};
  double ti[3], R[3][3], Ti[4][4], v1[4], v2[4], v3[4];
  pose::quat_rotate(qi, nt, ti);
  lba::quat_to_matrix(qi, R);
  VSG_SGBA_UNROLL
  for (int i = 0; i < 3; i++) {
    VSG_SGBA_UNROLL
    for (int j = 0; j < 3; j++) Ti[i][j] = R[i][j];
    Ti[i][3] = ti[i], Ti[3][i] = 0.0;
  }
  Ti[3][3] = 1.0;
  VSG_SGBA_UNROLL
  for (int c = 0; c < 4; c++) v1[c] = ((Pj[0] * Ti[0][c] + Pj[1] * Ti[1][c]) + Pj[2] * Ti[2][c]) + Pj[3] * Ti[3][c];
  VSG_SGBA_UNROLL
  for (int c = 0; c < 4; c++) v2[c] = ((v1[0] * G[c] + v1[1] * G[4 + c]) + v1[2] * G[8 + c]) + v1[3] * G[12 + c];
  VSG_SGBA_UNROLL
  for (int c = 0; c < 4; c++) v3[c] = ((v2[0] * Ti[c][0] + v2[1] * Ti[c][1]) + v2[2] * Ti[c][2]) + v2[3] * Ti[c][3];
  return ((v3[0] * Pj[0] + v3[1] * Pj[1]) + v3[2] * Pj[2]) + v3[3] * Pj[3];
}
// EdgeVertexPlaneProjectSE3KF: (kfPose * plane).ominus(measurement)
VSG_HD void plane_kf_error(const Est &T, const double *plane, const double *meas, double *e) {
  double local[4];
  plane_transform(T, plane, local);
  plane_ominus(local, meas, e);
}
// isDistanceCorrect of both plane edges (:319, :363)
VSG_HD bool distance_correct(const Est &T, const double *plane) {
  double local[4];
  plane_transform(T, plane, local);
  return local[3] > 0;
}
// the middle of two opposite walls, each turned by correctPlaneDirection first (:479-488, :537-545)
VSG_HD void wall_pair(const double *w1, const double *w2, double *vec) {
  double a[4], b[4];
  const bool fa = w1[3] > 0, fb = w2[3] > 0;
  VSG_SGBA_UNROLL
  for (int k = 0; k < 4; k++) a[k] = fa ? w1[k] * -1 : w1[k], b[k] = fb ? w2[k] * -1 : w2[k];
  const double da = __builtin_fabs(a[3]), db = __builtin_fabs(b[3]);
  VSG_SGBA_UNROLL
  for (int i = 0; i < 3; i++)
    vec[i] = da > db ? (0.5 * (da * a[i] - db * b[i])) + db * b[i] : (0.5 * (db * b[i] - da * a[i])) + da * a[i];
}

// ---- what the semantic phases index, beside lba::Prob.  Vertex 0 of an edge is its keyframe (plane edges) or its room;
// its local columns are 0-5, then three per plane.  An edge's quadratic form is stored edge-major: entry (a <= c) of the
// upper triangle over its local columns at [a * kMaxCols + c], b at [oB + a].
struct Sem {
  int32_t Pl, R, Pa, Es, n_obs, nsv, nsr, nbs, Ge0, Gp0, Gse, Gsr;
  const int32_t *e_kind, *e_v0, *e_obs, *e_fix0;  // [Es] kind; keyframe or room; observation (-1: a room edge); vertex 0 fixed
  const int32_t *e_pl;                             // [4 Es] the planes
  const double *e_w;                               // [Es] the information's diagonal
  const double *obs_local, *obs_G;                 // [4 n_obs] [16 n_obs]
  const int32_t *o_kf, *o_pl, *o_pk, *o_pp;        // [n_obs] keyframe, plane, the two edges (-1: not added)
  const int32_t *pl_act;                           // [Pl] index among the planes with an edge, -1: none
  const int32_t *sv_row, *sv_item;                 // [nsv] first row; plane (sv < Pa) or room
  const int32_t *row_sv;                           // [nsr]
  const int32_t *v_off, *v_edge, *v_col;           // [nsv + 1]: a semantic vertex's edges and its first column in each
  const int32_t *ks_off, *ks_edge;                 // [Ko + 1]: an optimised keyframe's semantic edges
  const int32_t *sb_s, *sb_t, *sb_off, *sb_edge, *sb_ca, *sb_cb;  // blocks (rows: semantic vertex s; columns t) and their lists
  double *pl[2];                                   // [4 Pl] each
  Est *rm[2];                                      // [R] each
  double *blocks, *chi2, *cost, *bsem;             // [kBlock Es] [Es] [Es] [nsr]
};

// The estimate buffers by a select, not by an index: indexing an array INSIDE a kernel argument with a run-time value makes
// the compiler copy the whole argument struct into scratch.
VSG_HD double *planes_of(const Sem &s, int buf) { return buf ? s.pl[1] : s.pl[0]; }
VSG_HD Est *rooms_of(const Sem &s, int buf) { return buf ? s.rm[1] : s.rm[0]; }
VSG_HD const Est *poses_of(const lba::Prob &p, int buf) { return buf ? p.est[1] : p.est[0]; }

struct EdgeInfo {
  int kind, npl, cols, dim;
  bool fix0;
  double w, delta;
};
VSG_HD EdgeInfo edge_info(const Sem &s, int e) {
  EdgeInfo I;
  I.kind = s.e_kind[e];
  I.npl = I.kind == kRoom4 ? 4 : I.kind == kRoom2 ? 2 : 1;
  I.cols = 6 + 3 * I.npl, I.dim = I.kind == kPointPlane ? 1 : 3;
  I.fix0 = s.e_fix0[e] != 0, I.w = s.e_w[e];
  I.delta = I.kind == kPointPlane ? (double)1.9598469734191895f : pose::huber_delta(true);  // thHuber1D, thHuberStereo
  return I;
}
// whether evaluation `slot` of an edge is made: 2 * column + (0: +delta, 1: -delta), 2 * cols = the error itself
VSG_HD bool slot_live(const EdgeInfo &I, int slot) { return slot <= 2 * I.cols && (slot >= 12 || !I.fix0); }

// computeError of edge e at estimate buffer buf with the oplus of `slot` applied (push, oplus, computeError, pop)
VSG_HD void slot_error(const lba::Prob &p, const Sem &s, int e, const EdgeInfo &I, int slot, int buf, double *err) {
  const int v0 = s.e_v0[e];
  Est T = I.kind <= kPlaneKf ? poses_of(p, buf)[v0] : rooms_of(s, buf)[v0];
  double W[4][4];
  VSG_SGBA_UNROLL
  for (int k = 0; k < 4; k++) {
    const double *src = planes_of(s, buf) + 4 * (size_t)s.e_pl[4 * (size_t)e + (k < I.npl ? k : 0)];
    VSG_SGBA_UNROLL
    for (int j = 0; j < 4; j++) W[k][j] = src[j];
  }
  if (slot < 2 * I.cols) {
    const int col = slot >> 1;
    const double d = (slot & 1) ? -1e-9 : 1e-9;
    if (col < 6) {
      double u[6];
      VSG_SGBA_UNROLL
      for (int k = 0; k < 6; k++) u[k] = k == col ? d : 0.0;
      T = pose::est_oplus(T, u);
    } else {
      const int which = (col - 6) / 3, a = (col - 6) % 3;
      double u[3], in[4], o[4];
      VSG_SGBA_UNROLL
      for (int k = 0; k < 3; k++) u[k] = k == a ? d : 0.0;
      VSG_SGBA_UNROLL
      for (int j = 0; j < 4; j++) in[j] = which == 0 ? W[0][j] : which == 1 ? W[1][j] : which == 2 ? W[2][j] : W[3][j];
      plane_oplus(in, u, o);
      VSG_SGBA_UNROLL
      for (int k = 0; k < 4; k++) {
        VSG_SGBA_UNROLL
        for (int j = 0; j < 4; j++) W[k][j] = k == which ? o[j] : W[k][j];
      }
    }
  }
  err[0] = err[1] = err[2] = 0.0;
  if (I.kind == kPointPlane) {
    err[0] = point_plane_error(T, W[0], s.obs_G + 16 * (size_t)s.e_obs[e]);
  } else if (I.kind == kPlaneKf) {
    plane_kf_error(T, W[0], s.obs_local + 4 * (size_t)s.e_obs[e], err);
  } else {
    double vx[3], vy[3] = {0.0, 0.0, 0.0};
    wall_pair(W[0], W[1], vx);
    if (I.kind == kRoom4) {
      wall_pair(W[2], W[3], vy);
      VSG_SGBA_UNROLL
      for (int i = 0; i < 3; i++) err[i] = T.t[i] - (vx[i] + vy[i]);
    } else {
      VSG_SGBA_UNROLL
      for (int i = 0; i < 3; i++) err[i] = T.t[i] - vx[i];
    }
  }
}
// column d of a Jacobian from its two slots' errors: errorBak = e+; errorBak -= e-; scalar * errorBak
VSG_HD double jacobian_entry(double ep, double em) { return (1.0 / (2 * 1e-9)) * (ep - em); }
// chi2() = error . (information * error), information = w I multiplied out with its zeros
VSG_HD double edge_chi2(const double *e, int dim, double w) {
  double c = 0.0;
  for (int r = 0; r < dim; r++) {
    double oe = 0.0;
    for (int k = 0; k < dim; k++) oe = oe + (k == r ? w : 0.0) * e[k];
    c = c + e[r] * oe;
  }
  return c;
}
// whether entry x of kBlock is written: both columns belong to the edge and to vertices that are not fixed
VSG_HD bool block_entry_live(const EdgeInfo &I, int x) {
  const int lo = I.fix0 ? 6 : 0;
  if (x >= oB) return x - oB >= lo && x - oB < I.cols;
  const int a = x / kMaxCols, c = x % kMaxCols;
  return a >= lo && a <= c && c < I.cols;
}
// entry x of an edge's quadratic form: J[r * kMaxCols + column], err, rho1 of the robust kernel
VSG_HD double block_entry(const double *J, const double *err, const EdgeInfo &I, double rho1, int x) {
  double sum = 0.0;
  if (x >= oB) {  // J^T omega_r, omega_r = -(omega * e) * rho1
    for (int r = 0; r < I.dim; r++) sum = sum + J[r * kMaxCols + (x - oB)] * (-(I.w * err[r]) * rho1);
    return sum;
  }
  const int a = x / kMaxCols, c = x % kMaxCols;
  const double wo = rho1 * I.w;
  for (int r = 0; r < I.dim; r++) sum = sum + (J[r * kMaxCols + a] * wo) * J[r * kMaxCols + c];
  return sum;
}
// the error of edge e as it stands: stores chi2, returns rho0; *rho1 = the kernel's weight
VSG_HD double edge_cost(const lba::Prob &p, const Sem &s, int e, int buf, double *err, double *rho1) {
  const EdgeInfo I = edge_info(s, e);
  slot_error(p, s, e, I, 2 * I.cols, buf, err);
  const double chi2 = edge_chi2(err, I.dim, I.w);
  s.chi2[e] = chi2;
  double rho0;
  pose::huber(chi2, I.delta, &rho0, rho1);
  return rho0;
}

// PHASE gather, semantic row r (0 = the first row behind the keyframes): b and the diagonal, serial over the vertex's edges.
// Returns |diagonal| for computeLambdaInit.
VSG_HD double gather_row(const Sem &s, int r, int n_kf_rows) {
  const int sv = s.row_sv[r], k = r - (s.sv_row[sv] - n_kf_rows);
  double b = 0.0, d = 0.0;
  for (int x = s.v_off[sv]; x < s.v_off[sv + 1]; x++) {
    const double *B = s.blocks + (size_t)s.v_edge[x] * kBlock;
    const int col = s.v_col[x] + k;
    b = b + B[oB + col], d = d + B[col * kMaxCols + col];
  }
  s.bsem[r] = b;
  return lba::max_diag(0.0, d);
}
// PHASE gather, optimised keyframe i: its semantic edges' blocks behind the visual sums of Hpp / bp, the maximum again
VSG_HD void gather_kf(const lba::Prob &p, const Sem &s, int i) {
  if (s.ks_off[i] == s.ks_off[i + 1]) return;
  double acc[lba::kHppC];
  for (int k = 0; k < lba::kHppC; k++) acc[k] = p.Hpp[(size_t)i * lba::kHppC + k];
  for (int x = s.ks_off[i]; x < s.ks_off[i + 1]; x++) {
    const double *B = s.blocks + (size_t)s.ks_edge[x] * kBlock;
    int h = 0;
    for (int a = 0; a < 6; a++)
      for (int c = a; c < 6; c++, h++) acc[h] = acc[h] + B[a * kMaxCols + c];
    for (int a = 0; a < 6; a++) acc[21 + a] = acc[21 + a] + B[oB + a];
  }
  lba::gather_kf_store(p, i, acc);
}
// PHASE trial, entry ent of block blk of the reduced system: rows = semantic vertex s, columns = keyframe t < Ko or
// semantic vertex t - Ko <= s.  A block without a contribution is written as zeros; lambda goes on the diagonal.
VSG_HD void assemble_entry(const lba::Prob &p, const Sem &s, int blk, int ent, double lambda) {
  const int sa = s.sb_s[blk], t = s.sb_t[blk], r = ent / 6, c = ent % 6;
  const int ra = s.sv_row[sa], da = sa < s.Pa ? 3 : 6;
  const bool kf = t < p.Ko, diag = !kf && t - p.Ko == sa;
  const int rb = kf ? 6 * t : s.sv_row[kf ? 0 : t - p.Ko], db = kf ? 6 : (t - p.Ko < s.Pa ? 3 : 6);
  if (r >= da || c >= db || (diag && c > r)) return;
  double sum = 0.0;
  for (int x = s.sb_off[blk]; x < s.sb_off[blk + 1]; x++) {
    const int la = s.sb_ca[x] + r, lb = s.sb_cb[x] + c;
    sum = sum + s.blocks[(size_t)s.sb_edge[x] * kBlock + (la < lb ? la * kMaxCols + lb : lb * kMaxCols + la)];
  }
  if (diag && r == c) sum = sum + lambda;
  p.M[(size_t)(ra + r) * p.n + (rb + c)] = sum;
}
// PHASE trial, semantic vertex sv: oplusImpl into the other buffer (VertexPlane: Plane3D::oplus; the room: SE3Quat::exp)
VSG_HD void oplus_vertex(const lba::Prob &p, const Sem &s, int sv, int cur) {
  const int item = s.sv_item[sv];
  const double *x = p.xp + s.sv_row[sv];
  if (sv < s.Pa)
    plane_oplus(planes_of(s, cur) + 4 * (size_t)item, x, planes_of(s, cur ^ 1) + 4 * (size_t)item);
  else
    rooms_of(s, cur ^ 1)[item] = pose::est_oplus(rooms_of(s, cur)[item], x);
}
// computeScale's term of semantic row r
VSG_HD double scale_row(const lba::Prob &p, const Sem &s, int r, double lambda) {
  const double x = p.xp[6 * p.Ko + r];
  return x * (lambda * x + s.bsem[r]);
}
// PHASE final, observation o: vToErasePlane (:2342-2369) as one flag, and the two chi2 compared
VSG_HD void classify_obs(const lba::Prob &p, const Sem &s, int o, int cur, uint8_t *erase, double *chi2_kf, double *chi2_pp) {
  const bool ok = distance_correct(poses_of(p, cur)[s.o_kf[o]], planes_of(s, cur) + 4 * (size_t)s.o_pl[o]);
  const int ek = s.o_pk[o], ep = s.o_pp[o];
  const double nan = __builtin_nan("");
  const double ck = ek >= 0 ? s.chi2[ek] : nan, cp = ep >= 0 ? s.chi2[ep] : nan;
  erase[o] = ((ek >= 0 && (ck > 7.815 || !ok)) || (ep >= 0 && (cp > 3.841 || !ok))) ? 1 : 0;
  if (chi2_kf) chi2_kf[o] = pose::canon(ck);
  if (chi2_pp) chi2_pp[o] = pose::canon(cp);
}

// ---- host only from here: the argument check and the lists (the library and the host core share them)

struct SemIn {
  int n_planes;
  const double *plane_eq;
  const int32_t *obs_off, *obs_kf;
  const double *obs_local, *obs_G, *w_kf, *w_pp;
  int n_rooms;
  const double *room_center;
  const int32_t *room_n_walls, *room_wall;
};

inline bool finite_d(double v) { return v - v == 0.0; }

// What vsg_mappoints_local_bundle_adjustment_sgraph checks of the new lists; kf_cnt[k] = plane edges of keyframe k,
// *n_pk / *n_pp = the edges of the two kinds (an edge with weight 0 is not added)
inline int check_lists(const SemIn &in, int n_kf, std::vector<int32_t> *kf_cnt, int *n_pk, int *n_pp) {
  *n_pk = *n_pp = 0;
  kf_cnt->assign((size_t)(n_kf > 0 ? n_kf : 0), 0);
  if (in.n_planes < 0 || in.n_rooms < 0) return VSG_ERR_INVALID;
  int n_obs = 0;
  if (in.n_planes > 0) {
    if (!in.plane_eq || !in.obs_off || in.obs_off[0] != 0) return VSG_ERR_INVALID;
    for (int i = 0; i < in.n_planes; i++)
      if (in.obs_off[i + 1] < in.obs_off[i]) return VSG_ERR_INVALID;
    n_obs = in.obs_off[in.n_planes];
    if (n_obs > 0 && (!in.obs_kf || !in.obs_local || !in.obs_G || !in.w_kf || !in.w_pp)) return VSG_ERR_INVALID;
    std::vector<int32_t> seen((size_t)(n_kf > 0 ? n_kf : 0), -1);
    for (int i = 0; i < in.n_planes; i++) {
      const double *c = in.plane_eq + 4 * (size_t)i;
      if (!finite_d(c[0]) || !finite_d(c[1]) || !finite_d(c[2]) || !finite_d(c[3])) return VSG_ERR_INVALID;
      if (c[0] == 0.0 && c[1] == 0.0 && c[2] == 0.0) return VSG_ERR_INVALID;
      for (int o = in.obs_off[i]; o < in.obs_off[i + 1]; o++) {
        const int k = in.obs_kf[o];
        if (k < 0 || k >= n_kf || seen[(size_t)k] == i) return VSG_ERR_INVALID;
        seen[(size_t)k] = i;
        if (!(in.w_kf[o] >= 0.0) || !(in.w_pp[o] >= 0.0)) return VSG_ERR_INVALID;
        if (in.w_kf[o] > 0.0) (*kf_cnt)[(size_t)k]++, (*n_pk)++;
        if (in.w_pp[o] > 0.0) (*kf_cnt)[(size_t)k]++, (*n_pp)++;
      }
    }
  }
  if (in.n_rooms > 0) {
    if (!in.room_center || !in.room_n_walls || !in.room_wall) return VSG_ERR_INVALID;
    for (int r = 0; r < in.n_rooms; r++) {
      const int nw = in.room_n_walls[r];
      if (nw != 2 && nw != 4) return VSG_ERR_INVALID;
      for (int a = 0; a < nw; a++) {
        const int wa = in.room_wall[4 * (size_t)r + a];
        if (wa < 0 || wa >= in.n_planes) return VSG_ERR_INVALID;
        for (int b = 0; b < a; b++)
          if (in.room_wall[4 * (size_t)r + b] == wa) return VSG_ERR_INVALID;
      }
    }
  }
  return VSG_OK;
}

struct SemTopology {
  int Pl = 0, R = 0, Pa = 0, Es = 0, n_obs = 0, nsv = 0, nsr = 0, nbs = 0, n = 0, n_pk = 0, n_pp = 0;
  std::vector<int32_t> e_kind, e_v0, e_obs, e_fix0, e_pl, o_kf, o_pl, o_pk, o_pp, pl_act, sv_row, sv_item, row_sv, v_off, v_edge,
      v_col, ks_off, ks_edge, sb_s, sb_t, sb_off, sb_edge, sb_ca, sb_cb;
  std::vector<double> e_w;
};

// The semantic edges and every list the phases walk, after lba::check_and_build has named the optimised keyframes.
// VSG_ERR_UNSUPPORTED: more than kMaxRows rows.
inline int build_lists(const lba::Topology &T, const SemIn &in, SemTopology *S) {
  const int Pl = in.n_planes, R = in.n_rooms, Ko = T.Ko;
  S->Pl = Pl, S->R = R, S->n_obs = Pl > 0 ? in.obs_off[Pl] : 0;
  const size_t NO = (size_t)S->n_obs;
  S->o_kf.assign(NO, 0), S->o_pl.assign(NO, 0), S->o_pk.assign(NO, -1), S->o_pp.assign(NO, -1);
  S->pl_act.assign((size_t)Pl, -1);
  S->e_kind.clear(), S->e_v0.clear(), S->e_obs.clear(), S->e_fix0.clear(), S->e_pl.clear(), S->e_w.clear();
  std::vector<uint8_t> used((size_t)Pl, 0);
  auto add_edge = [&](int kind, int v0, int obs, bool fix0, const int32_t *pl, int npl, double w) {
    S->e_kind.push_back(kind), S->e_v0.push_back(v0), S->e_obs.push_back(obs), S->e_fix0.push_back(fix0 ? 1 : 0), S->e_w.push_back(w);
    for (int k = 0; k < 4; k++) S->e_pl.push_back(k < npl ? pl[k] : 0);
    for (int k = 0; k < npl; k++) used[(size_t)pl[k]] = 1;
    return (int32_t)S->e_kind.size() - 1;
  };
  S->n_pk = S->n_pp = 0;
  for (int i = 0; i < Pl; i++)
    for (int o = in.obs_off[i]; o < in.obs_off[i + 1]; o++) {
      const int k = in.obs_kf[o];
      const int32_t pl = i;
      const bool fixed = T.opt_of[(size_t)k] < 0;
      S->o_kf[(size_t)o] = k, S->o_pl[(size_t)o] = i;
      if (in.w_kf[o] > 0.0) S->o_pk[(size_t)o] = add_edge(kPlaneKf, k, o, fixed, &pl, 1, in.w_kf[o]), S->n_pk++;
      if (in.w_pp[o] > 0.0) S->o_pp[(size_t)o] = add_edge(kPointPlane, k, o, fixed, &pl, 1, in.w_pp[o]), S->n_pp++;
    }
  for (int r = 0; r < R; r++) {
    const int nw = in.room_n_walls[r];
    add_edge(nw == 4 ? kRoom4 : kRoom2, r, -1, false, in.room_wall + 4 * (size_t)r, nw, 1.0);
  }
  S->Es = (int)S->e_kind.size();
  // the semantic vertices: the planes with an edge in list order, then the rooms
  S->Pa = 0;
  S->sv_row.clear(), S->sv_item.clear(), S->row_sv.clear();
  int row = 6 * Ko;
  for (int i = 0; i < Pl; i++)
    if (used[(size_t)i]) {
      S->pl_act[(size_t)i] = S->Pa++, S->sv_row.push_back(row), S->sv_item.push_back(i);
      for (int k = 0; k < 3; k++) S->row_sv.push_back((int32_t)S->sv_row.size() - 1);
      row += 3;
    }
  for (int r = 0; r < R; r++) {
    S->sv_row.push_back(row), S->sv_item.push_back(r);
    for (int k = 0; k < 6; k++) S->row_sv.push_back((int32_t)S->sv_row.size() - 1);
    row += 6;
  }
  S->nsv = (int)S->sv_row.size(), S->n = row, S->nsr = row - 6 * Ko;
  if (S->n > kMaxRows) return VSG_ERR_UNSUPPORTED;
  // per edge: its vertices as (block vertex, first local column); block vertex = optimised keyframe i, or Ko + semantic vertex
  const int nsv = S->nsv, Es = S->Es;
  auto base = [Ko](int s) { return s * Ko + s * (s + 1) / 2; };
  S->nbs = base(nsv);
  S->sb_s.resize((size_t)S->nbs), S->sb_t.resize((size_t)S->nbs);
  for (int s = 0; s < nsv; s++)
    for (int t = 0; t < Ko + s + 1; t++) S->sb_s[(size_t)(base(s) + t)] = s, S->sb_t[(size_t)(base(s) + t)] = t;
  S->sb_off.assign((size_t)S->nbs + 1, 0), S->v_off.assign((size_t)nsv + 1, 0), S->ks_off.assign((size_t)Ko + 1, 0);
  for (int pass = 0; pass < 2; pass++) {
    std::vector<int32_t> at_b(S->sb_off.begin(), S->sb_off.end() - 1), at_v(S->v_off.begin(), S->v_off.end() - 1),
        at_k(S->ks_off.begin(), S->ks_off.end() - 1);
    for (int e = 0; e < Es; e++) {
      const int kind = S->e_kind[(size_t)e], npl = kind == kRoom4 ? 4 : kind == kRoom2 ? 2 : 1;
      int vert[5], col[5], nv = 0;
      if (kind <= kPlaneKf) {
        const int o = T.opt_of[(size_t)S->e_v0[(size_t)e]];
        if (o >= 0) {
          vert[nv] = o, col[nv] = 0, nv++;
          if (pass == 0)
            S->ks_off[(size_t)o + 1]++;
          else
            S->ks_edge[(size_t)at_k[(size_t)o]++] = e;
        }
      } else {
        vert[nv] = Ko + S->Pa + S->e_v0[(size_t)e], col[nv] = 0, nv++;
      }
      for (int k = 0; k < npl; k++) vert[nv] = Ko + S->pl_act[(size_t)S->e_pl[4 * (size_t)e + k]], col[nv] = 6 + 3 * k, nv++;
      for (int a = 0; a < nv; a++) {
        if (vert[a] < Ko) continue;
        const int sa = vert[a] - Ko;
        if (pass == 0)
          S->v_off[(size_t)sa + 1]++;
        else
          S->v_edge[(size_t)at_v[(size_t)sa]] = e, S->v_col[(size_t)at_v[(size_t)sa]] = col[a], at_v[(size_t)sa]++;
        for (int b = 0; b < nv; b++) {
          if (vert[b] > vert[a]) continue;  // the block's columns are the vertex of the lower row (or the same one)
          const size_t B = (size_t)(base(sa) + vert[b]);
          if (pass == 0)
            S->sb_off[B + 1]++;
          else
            S->sb_edge[(size_t)at_b[B]] = e, S->sb_ca[(size_t)at_b[B]] = col[a], S->sb_cb[(size_t)at_b[B]] = col[b], at_b[B]++;
        }
      }
    }
    if (pass == 0) {
      for (int b = 0; b < S->nbs; b++) S->sb_off[(size_t)b + 1] += S->sb_off[(size_t)b];
      for (int v = 0; v < nsv; v++) S->v_off[(size_t)v + 1] += S->v_off[(size_t)v];
      for (int k = 0; k < Ko; k++) S->ks_off[(size_t)k + 1] += S->ks_off[(size_t)k];
      S->sb_edge.resize((size_t)S->sb_off[(size_t)S->nbs]), S->sb_ca.resize(S->sb_edge.size()), S->sb_cb.resize(S->sb_edge.size());
      S->v_edge.resize((size_t)S->v_off[(size_t)nsv]), S->v_col.resize(S->v_edge.size());
      S->ks_edge.resize((size_t)S->ks_off[(size_t)Ko]);
    }
  }
  return VSG_OK;
}

// The argument check of the whole call, the visual lists and the semantic ones.  *ran = 0 with VSG_OK: the reference
// returned before optimize (:1734, :2277 -- nEdges counts the visual and the plane edges, never a room's -- :2283) or
// n_points == 0.
template <class OctaveOf>
inline int check_and_build(int n_points, const int32_t *slots, const int32_t *obs_off, const int32_t *obs_kf,
                           const int32_t *obs_idx, int n_kf, const int32_t *kf_n, const int32_t *nleft, OctaveOf octave,
                           const uint8_t *kf_fixed, int capacity, int nlevels, int iterations,
                           const volatile uint8_t *stop_flag, const SemIn &in, lba::Topology *T, SemTopology *S, int *ran) {
  *ran = 0;
  if (n_kf < 0) return VSG_ERR_INVALID;
  std::vector<int32_t> kf_cnt;
  int rc = check_lists(in, n_kf, &kf_cnt, &S->n_pk, &S->n_pp);
  if (rc != VSG_OK) return rc;
  rc = lba::check_and_build(n_points, slots, obs_off, obs_kf, obs_idx, n_kf, kf_n, nleft, octave, kf_fixed, capacity, nlevels,
                            iterations, nullptr, T, ran, lba::kMaxOptKf, true, kf_cnt.data(), S->n_pk + S->n_pp);
  if (rc != VSG_OK || !*ran) return rc;
  *ran = 0;
  rc = build_lists(*T, in, S);
  if (rc != VSG_OK) return rc;
  if (stop_flag && *stop_flag) return VSG_OK;  // :2283
  *ran = 1;
  return VSG_OK;
}

inline void fill_result(vsg_sgraph_local_ba_result *res, const lba::Topology &T, const SemTopology *ST, const lba::State *S) {
  memset(res, 0, sizeof(*res));
  lba::fill_result(&res->local, T, S);
  if (!S) return;
  res->n_planes_active = ST->Pa, res->n_rooms_active = ST->R, res->n_plane_kf = ST->n_pk, res->n_plane_point = ST->n_pp;
  res->n_room_edges = ST->R, res->n_rows = ST->n;
}

// The start values of the semantic vertices as both estimate buffers take them (:2028-2029, :2171-2172)
inline void start_values(const SemIn &in, double *pl0, double *pl1, Est *rm0, Est *rm1) {
  for (size_t k = 0; k < 4 * (size_t)in.n_planes; k++) pl0[k] = pl1[k] = in.plane_eq[k];
  for (int r = 0; r < in.n_rooms; r++) {
    Est e;
    e.q[0] = e.q[1] = e.q[2] = 0.0, e.q[3] = 1.0;
    for (int k = 0; k < 3; k++) e.t[k] = in.room_center[3 * (size_t)r + k];
    rm0[r] = rm1[r] = e;
  }
}
// the pointers of Sem that name lists, from a SemTopology that outlives it
inline void point_lists(Sem *s, const SemTopology &S, const SemIn &in, int Ge0, int Gp0) {
  memset(s, 0, sizeof(*s));
  s->Pl = S.Pl, s->R = S.R, s->Pa = S.Pa, s->Es = S.Es, s->n_obs = S.n_obs, s->nsv = S.nsv, s->nsr = S.nsr, s->nbs = S.nbs;
  s->Ge0 = Ge0, s->Gp0 = Gp0, s->Gse = (S.Es + lba::kThreads - 1) / lba::kThreads, s->Gsr = (S.nsr + lba::kThreads - 1) / lba::kThreads;
  s->e_kind = S.e_kind.data(), s->e_v0 = S.e_v0.data(), s->e_obs = S.e_obs.data(), s->e_fix0 = S.e_fix0.data(), s->e_pl = S.e_pl.data();
  s->e_w = S.e_w.data(), s->obs_local = in.obs_local, s->obs_G = in.obs_G, s->o_kf = S.o_kf.data(), s->o_pl = S.o_pl.data();
  s->o_pk = S.o_pk.data(), s->o_pp = S.o_pp.data(), s->pl_act = S.pl_act.data(), s->sv_row = S.sv_row.data(), s->sv_item = S.sv_item.data();
  s->row_sv = S.row_sv.data(), s->v_off = S.v_off.data(), s->v_edge = S.v_edge.data(), s->v_col = S.v_col.data();
  s->ks_off = S.ks_off.data(), s->ks_edge = S.ks_edge.data(), s->sb_s = S.sb_s.data(), s->sb_t = S.sb_t.data(), s->sb_off = S.sb_off.data();
  s->sb_edge = S.sb_edge.data(), s->sb_ca = S.sb_ca.data(), s->sb_cb = S.sb_cb.data();
}

// The whole call on the host, phase by phase as vsg_sgraph_ba.hip enqueues them, every sum in the device's tree.
struct HostRun {
  lba::HostRun V;  // the visual part: its lists, estimates and per-edge blocks
  SemTopology ST;
  Sem s;
  lba::Prob pc;  // V.p as the controller sees it: the semantic partials behind the visual ones
  std::vector<double> pl[2], blocks, chi2, cost, bsem, M, bs, xp, chiPart, maxPart, scalePart;
  std::vector<Est> rm[2];

  // after V.T and ST are set; the visual arguments are lba::HostRun::setup's
  void setup(const float *pos, const float *kx, const float *ky, const float *ur, const int32_t *oct, const vsg_pose_se3 *Tcw,
             const uint8_t *fixed, const vsg_ba_camera *kc, const float *sig, int nlevels, int iterations, const SemIn &in) {
    V.setup(pos, kx, ky, ur, oct, Tcw, fixed, kc, sig, nlevels, iterations);
    lba::Prob &p = V.p;
    point_lists(&s, ST, in, p.Ge, p.Gp);
    const size_t n = (size_t)ST.n, Es = (size_t)ST.Es;
    for (int b = 0; b < 2; b++) pl[b].resize(4 * (size_t)ST.Pl), rm[b].resize((size_t)ST.R);
    start_values(in, pl[0].data(), pl[1].data(), rm[0].data(), rm[1].data());
    blocks.assign(kBlock * Es, 0.0), chi2.assign(Es, 0.0), cost.assign(Es, 0.0), bsem.assign((size_t)ST.nsr, 0.0);
    M.assign(n * n, 0.0), bs.assign(n, 0.0), xp.assign(n, 0.0);
    chiPart.assign((size_t)(s.Ge0 + s.Gse), 0.0), maxPart.assign((size_t)(s.Gp0 + s.Gsr), 0.0), scalePart.assign((size_t)(s.Gp0 + s.Gsr), 0.0);
    for (int b = 0; b < 2; b++) s.pl[b] = pl[b].data(), s.rm[b] = rm[b].data();
    s.blocks = blocks.data(), s.chi2 = chi2.data(), s.cost = cost.data(), s.bsem = bsem.data();
    p.n = ST.n, p.M = M.data(), p.bs = bs.data(), p.xp = xp.data();
    p.chiPart = chiPart.data(), p.maxPart = maxPart.data(), p.scalePart = scalePart.data();
    pc = p;
    pc.Ge = s.Ge0 + s.Gse, pc.Gp = s.Gp0 + s.Gsr;
  }
  // one wave of the device's linearise kernel: the evaluations side by side, then the edge's blocks
  void linearise_edge(int e, int buf) {
    const lba::Prob &p = V.p;
    const EdgeInfo I = edge_info(s, e);
    double err[kMaxSlots][3], J[3 * kMaxCols];
    for (int slot = 0; slot <= 2 * I.cols; slot++)
      if (slot_live(I, slot)) slot_error(p, s, e, I, slot, buf, err[slot]);
    for (int x = 0; x < 3 * kMaxCols; x++) {
      const int r = x / kMaxCols, c = x % kMaxCols;
      J[x] = c < I.cols && slot_live(I, 2 * c) ? jacobian_entry(err[2 * c][r], err[2 * c + 1][r]) : 0.0;
    }
    const double *e0 = err[2 * I.cols];
    const double c2 = edge_chi2(e0, I.dim, I.w);
    double rho0, rho1;
    pose::huber(c2, I.delta, &rho0, &rho1);
    s.chi2[e] = c2, s.cost[e] = rho0;
    for (int x = 0; x < kBlock; x++)
      if (block_entry_live(I, x)) s.blocks[(size_t)e * kBlock + x] = block_entry(J, e0, I, rho1, x);
  }
  void max_rows() {
    for (int g = 0; g < s.Gsr; g++) {
      double v[lba::kThreads];
      for (int t = 0; t < lba::kThreads; t++) v[t] = g * lba::kThreads + t < s.nsr ? gather_row(s, g * lba::kThreads + t, 6 * V.p.Ko) : 0.0;
      maxPart[(size_t)(s.Gp0 + g)] = lba::HostRun::max_tree(v);
    }
  }
  void error_pass(int buf) {
    V.grouped(V.p.E, chiPart.data(), [&](int e) {
      double err[3], Xc[3], rho1;
      return lba::edge_cost(V.p, e, buf, err, Xc, &rho1);
    });
    V.grouped(s.Es, chiPart.data() + s.Ge0, [&](int e) {
      double err[3], rho1;
      return edge_cost(V.p, s, e, buf, err, &rho1);
    });
  }
  void run(const volatile uint8_t *stop_flag) {
    const lba::Prob &p = V.p;
    lba::State &S = V.S;
    for (int it = 0; it < p.iterations; it++) {
      if (!lba::run_iteration(S, it)) break;
      V.grouped(p.E, chiPart.data(), [&](int e) { return lba::linearise_edge(p, e, S.cur); });
      for (int e = 0; e < s.Es; e++) linearise_edge(e, S.cur);
      V.grouped(s.Es, chiPart.data() + s.Ge0, [&](int e) { return s.cost[e]; });
      for (int g = 0; g < s.Gp0; g++) {
        double v[lba::kThreads];
        for (int t = 0; t < lba::kThreads; t++) v[t] = g * lba::kThreads + t < p.P ? lba::gather_point(p, g * lba::kThreads + t) : 0.0;
        maxPart[(size_t)g] = lba::HostRun::max_tree(v);
      }
      for (int i = 0; i < p.Ko; i++) {
        static thread_local double part[lba::kThreads][lba::kHppC];
        double acc[lba::kHppC];
        for (int t = 0; t < lba::kThreads; t++) lba::gather_kf_partial(p, i, t, part[t]);
        pose::HostTeam::tree<lba::kHppC>(part, lba::kHppC, acc);
        lba::gather_kf_store(p, i, acc);
      }
      max_rows();
      for (int i = 0; i < p.Ko; i++) gather_kf(p, s, i);
      lba::begin_iteration(pc, it);
      for (int q = 0; q < lba::kTrials; q++) {
        if (!lba::run_trial(S, it, q)) break;
        const double lambda = S.lambda;
        const int cur = S.cur;
        for (int e = 0; e < p.E; e++) lba::trial_edge(p, e, lambda);
        for (int b = 0; b < p.nb; b++)
          for (int r = 0; r < 6; r++)
            for (int cc = 0; cc < 6; cc++) lba::schur_entry(p, b, r, cc, lambda);
        for (int i = 0; i < p.Ko; i++) {
          static thread_local double part[lba::kThreads][lba::kC];
          double acc[lba::kC];
          for (int t = 0; t < lba::kThreads; t++) lba::bschur_partial(p, i, t, part[t]);
          pose::HostTeam::tree<lba::kC>(part, lba::kC, acc);
          lba::bschur_store(p, i, acc);
        }
        for (int b = 0; b < s.nbs; b++)
          for (int ent = 0; ent < 36; ent++) assemble_entry(p, s, b, ent, lambda);
        for (int r = 0; r < s.nsr; r++) p.bs[6 * p.Ko + r] = s.bsem[r];
        V.ok2 = lba::solve_reduced_host(p.n, p.M, p.bs, p.xp) ? 1 : 0;
        V.grouped(p.P, scalePart.data(), [&](int pt) { return lba::backsub_point(p, pt, cur, lambda); });
        for (int i = 0; i < p.Ko; i++) lba::oplus_kf(p, i, cur);
        for (int sv = 0; sv < s.nsv; sv++) oplus_vertex(p, s, sv, cur);
        V.grouped(s.nsr, scalePart.data() + s.Gp0, [&](int r) { return scale_row(p, s, r, lambda); });
        error_pass(cur ^ 1);
        lba::decide(pc);
      }
      if (!S.finished && stop_flag && *stop_flag) S.finished = 1, S.stop_reason = lba::kStopFlag;
    }
  }
  // the semantic outs; the visual ones are V.outputs.  A plane without an edge keeps its input bytes (g2o drops the vertex).
  void outputs(const SemIn &in, double *plane_eq_out, double *room_center_out, uint8_t *erase_plane, double *chi2_kf, double *chi2_pp) {
    const int cur = V.S.cur;
    for (int o = 0; o < s.n_obs; o++) classify_obs(V.p, s, o, cur, erase_plane, chi2_kf, chi2_pp);
    for (int i = 0; i < s.Pl; i++)
      for (int k = 0; k < 4; k++)
        plane_eq_out[4 * (size_t)i + k] = ST.pl_act[(size_t)i] >= 0 ? pose::canon(pl[cur][4 * (size_t)i + k]) : in.plane_eq[4 * (size_t)i + k];
    for (int r = 0; r < s.R; r++)
      for (int k = 0; k < 3; k++) room_center_out[3 * (size_t)r + k] = pose::canon(rm[cur][(size_t)r].t[k]);
  }
};

}  // namespace sgba
}  // namespace vsg
