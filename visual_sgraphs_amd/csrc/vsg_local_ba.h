// vsg_local_ba.h -- the visual part of Optimizer::LocalBundleAdjustment (Optimizer.cc:1454-2454): keyframe poses, map
// points, monocular and stereo reprojection edges, host and device from one source.  The kernels of vsg_local_ba.hip run
// the per-item functions below over the whole chip; tests/_localbacore and the latency probe's caller-side loop compile the
// same functions for the host and replay every sum in the same tree (HostRun).
//
// Everything is double, as g2o has it.  What is restated, and from where:
//   * EdgeSE3ProjectXYZ (OptimizableTypes.h:96-, linearizeOplus OptimizableTypes.cpp:135-161) through Pinhole::project /
//     projectJac, and g2o::EdgeStereoSE3ProjectXYZ (types_six_dof_expmap.h:150-, cam_project .cpp:202-214 with its float
//     1 / z, linearizeOplus .cpp:248-297): error, isDepthPositive, both Jacobian blocks, information = invSigma2 * I;
//   * RobustKernelHuber (robust_kernel_impl.cpp:78) with the float deltas of :1847-1848 and constructQuadraticForm of
//     base_binary_edge.hpp:55-116, including its fixed pose vertex (no Hpp, no Hpl, the point's blocks alone);
//   * BlockSolver::buildSystem (block_solver.hpp:502-560): Hpp 6x6 per optimised keyframe, Hll 3x3 per point, Hpl 6x3 per
//     edge of an optimised keyframe, b;
//   * setLambda / solve / restoreDiagonal (:354-486, :564-605): lambda on both diagonals, Dinv = (Hll + lambda I)^-1,
//     Hschur = Hpp - sum (B Dinv) B^T, bschur = bp - sum B Dinv bl, the reduced solve, xl = Dinv (bl - B^T xp);
//   * OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale (optimization_algorithm_levenberg.cpp:
//     61-199) with the _nBad >= 3 stop, push / pop as two estimate buffers and an index;
//   * the classification (:2296-2340) with e->chi2() as the LAST computeActiveErrors left it and isDepthPositive on the
//     restored estimates, and the recovery (:2398-2414).
// SE3Quat exp / multiply / map, sin / cos and the pinhole error come from vsg_pose_opt.h.
//
// THE REDUCED SOLVE is a dense LDL^T without pivoting in the order the keyframes were given (the reference: Eigen's
// SimplicialLDLT behind an AMD ordering, linear_solver_eigen.h:94-124; equal to rounding on a positive-definite system).
// A pivot <= 0 gives ok2 = false and tempChi = DBL_MAX (optimization_algorithm_levenberg.cpp:126-127).  Element (i, j)
// takes its updates -(L_ik L_jk) D_k in ascending k on both sides, whatever the loop nest around it.
//
// ORDERS.  Edges are point-major in the caller's point order and inside a point in its list's order (g2o's insertion
// order); poses in the reduced system follow the keyframe array.  Every sum over edges is one fixed tree:
//   * a point's Hll / bl: serial over its edges;
//   * a keyframe's Hpp / bp, and its bschur: lane t of kThreads sums the keyframe's edges t, t + kThreads, ... serially,
//     then pose::HostTeam::tree (butterfly over each wave, the waves serially);
//   * a Schur entry: serial over the block's pair list, which the host builds in point order;
//   * the robust chi2, computeScale's point part and the lambda-init maximum: group g of kThreads consecutive items
//     through the same tree to one partial, the partials serially.
// No floating-point atomics.  Both builds use -ffp-contract=off.
//
// Every loop bound is a compile-time constant or a count the host validated: no input keeps a kernel running.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/vsg_orb.h"
#include "vsg_pose_opt.h"

namespace vsg {
namespace lba {

enum { kThreads = 256, kMaxOptKf = 128, kTrials = 10, kSolveThreads = 1024, kSolveTile = 32 };
enum { kStereo = 1 };                                                       // edge flag
enum { kStopIterations = 0, kStopTerminate = 1, kStopBad = 2, kStopFlag = 3 };  // vsg_local_ba_result.stop_reason
enum { kHpl = 18, kHppC = 27, kHllC = 9, kC = 6 };  // doubles per edge: Hpl 6x3 | Hpp upper 21 + bp 6 | Hll upper 6 + bl 3

using pose::Cam;
using pose::Est;

// The Levenberg controller.  Written by begin_iteration and decide (one lane each); every phase reads it first.
struct State {
  double lambda, ni, currentChi, iniChi, tempChi, rho, chi2_initial;
  int32_t iter, qmax, n_bad, finished, trial_open, cur, stop_reason, iterations_run, trials_run, n_mono, n_stereo, pad;
};

// What the phases index.  The blocks an edge's OWN lane reads and writes (obs, HppC, HllC, c) are structure-of-arrays:
// entry k of edge e is at [k * E + e].  Hpl and BDinv, which a Schur block's lanes and a point's lane read edge by edge, are
// arrays of structures: edge e's 18 doubles at [18 e].
struct Prob {
  int32_t K, Ko, P, E, n, nb, Ge, Gp, iterations;
  // topology, built and bounded by the host (Topology below)
  const int32_t *e_kf, *e_pt, *e_opt;  // [E] keyframe, point, index among the optimised keyframes (-1: fixed)
  const int32_t *p_off;                // [P + 1] the caller's obs_off
  const int32_t *k_off, *k_edge;       // [Ko + 1], the edges of optimised keyframe i ascending
  const int32_t *b_i, *b_j, *b_off;    // [nb], [nb], [nb + 1]: Schur block (i <= j) and its pair list
  const int32_t *pair_a, *pair_b;      // the edge in keyframe i, the edge in keyframe j, of one point
  const int32_t *opt_kf;               // [Ko] keyframe of optimised index i
  const Cam *cam;                      // [K]
  double *obs, *w;                     // [3 E], [E]
  uint8_t *flag;                       // [E]
  Est *est[2];                         // [K] each: current = est[S->cur]
  double *X[2];                        // [3 P] each
  double *chi2;                        // [E] as the last error pass left it
  double *Hpl, *HppC, *HllC, *BDinv, *c;  // [18 E] [27 E] [9 E] [18 E] [6 E]
  double *Hpp;                            // [27 Ko]: upper triangle row by row, then bp
  double *Hll;                            // [9 P]: upper triangle, then bl
  double *M, *bs, *xp;                    // [n n] row-major (lower triangle used), [n], [n]
  double *chiPart, *maxPart, *maxKf, *scalePart;  // [Ge] [Gp] [Ko] [Gp]
  int32_t *ok2;
  State *S;
};

VSG_HD bool run_iteration(const State &S, int it) { return !S.finished && S.iter == it; }
VSG_HD bool run_trial(const State &S, int it, int q) { return !S.finished && S.iter == it && S.trial_open && S.qmax == q; }

// Eigen's Quaternion::toRotationMatrix
VSG_HD void quat_to_matrix(const double *q, double R[3][3]) {
  const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3], txx = tx * q[0], txy = ty * q[0], txz = tz * q[0],
               tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0][0] = 1.0 - (tyy + tzz), R[0][1] = txy - twz, R[0][2] = txz + twy;
  R[1][0] = txy + twz, R[1][1] = 1.0 - (txx + tzz), R[1][2] = tyz - twx;
  R[2][0] = txz - twy, R[2][1] = tyz + twx, R[2][2] = 1.0 - (txx + tyy);
}

// linearizeOplus of both edges: A = d error / d point (rows x 3), B = d error / d pose (rows x 6)
VSG_HD void edge_jacobians(const Cam &K, const Est &T, const double *Xc, bool stereo, double A[3][3], double B[3][6]) {
  double R[3][3];
  quat_to_matrix(T.q, R);
  const double x = Xc[0], y = Xc[1], z = Xc[2];
  if (!stereo) {
    pose::edge_jacobian(K, Xc, false, B);  // -projectJac * SE3deriv
    // -pCamera->projectJac(xyz_trans) * T.rotation().toRotationMatrix(), summed in k order with its zero terms
    const double Pn[2][3] = {{-(K.fx / z), -0.0, -(-K.fx * x / (z * z))}, {-0.0, -(K.fy / z), -(-K.fy * y / (z * z))}};
    for (int i = 0; i < 2; i++)
      for (int j = 0; j < 3; j++) A[i][j] = (Pn[i][0] * R[0][j] + Pn[i][1] * R[1][j]) + Pn[i][2] * R[2][j];
    for (int j = 0; j < 3; j++) A[2][j] = 0.0;
    return;
  }
  const double z_2 = z * z;
  for (int j = 0; j < 3; j++) {
    A[0][j] = -K.fx * R[0][j] / z + K.fx * x * R[2][j] / z_2;
    A[1][j] = -K.fy * R[1][j] / z + K.fy * y * R[2][j] / z_2;
    A[2][j] = A[0][j] - K.bf * R[2][j] / z_2;
  }
  B[0][0] = x * y / z_2 * K.fx;
  B[0][1] = -(1 + (x * x / z_2)) * K.fx;
  B[0][2] = y / z * K.fx;
  B[0][3] = -1. / z * K.fx;
  B[0][4] = 0;
  B[0][5] = x / z_2 * K.fx;
  B[1][0] = (1 + y * y / z_2) * K.fy;
  B[1][1] = -x * y / z_2 * K.fy;
  B[1][2] = -x / z * K.fy;
  B[1][3] = 0;
  B[1][4] = -1. / z * K.fy;
  B[1][5] = y / z_2 * K.fy;
  B[2][0] = B[0][0] - K.bf * y / z_2;
  B[2][1] = B[0][1] + K.bf * x / z_2;
  B[2][2] = B[0][2];
  B[2][3] = B[0][3];
  B[2][4] = 0;
  B[2][5] = B[0][5] - K.bf / z_2;
}

VSG_HD pose::Edge edge_of(const Prob &p, int e, const double *X) {
  pose::Edge E;
  const int pt = p.e_pt[e];
  E.X[0] = X[3 * pt], E.X[1] = X[3 * pt + 1], E.X[2] = X[3 * pt + 2];
  E.obs[0] = p.obs[e], E.obs[1] = p.obs[(size_t)p.E + e], E.obs[2] = p.obs[2 * (size_t)p.E + e];
  E.w = p.w[e], E.chi2 = 0.0;
  return E;
}

// The robust kernel of the local call: Huber with the float deltas of :1847-1848 on every edge.  edge_cost and
// linearise_edge take the kernel as a type so that vsg_global_ba.h can pass one that is optional (bRobust) and has its own
// deltas; with this default they compile to the operations they always had.
struct HuberLocal {
  VSG_HD void operator()(double chi2, bool stereo, double *rho0, double *rho1) const {
    pose::huber(chi2, pose::huber_delta(stereo), rho0, rho1);
  }
};

// computeError + the robust cost of edge e at estimate buffer `buf`; stores chi2[e]
template <class Kernel = HuberLocal>
VSG_HD double edge_cost(const Prob &p, int e, int buf, double *err, double *Xc, double *rho1, const Kernel &kernel = Kernel()) {
  const bool stereo = (p.flag[e] & kStereo) != 0;
  const pose::Edge E = edge_of(p, e, p.X[buf]);
  const int kf = p.e_kf[e];
  const double chi2 = pose::edge_error(p.cam[kf], p.est[buf][kf], E, stereo, err, Xc);
  p.chi2[e] = chi2;
  double rho0;
  kernel(chi2, stereo, &rho0, rho1);
  return rho0;
}

// PHASE linearise, one edge: linearizeOplus + constructQuadraticForm into the edge's own blocks.  Returns rho0.
template <class Kernel = HuberLocal>
VSG_HD double linearise_edge(const Prob &p, int e, int buf, const Kernel &kernel = Kernel()) {
  double err[3], Xc[3], rho1;
  const double rho0 = edge_cost(p, e, buf, err, Xc, &rho1, kernel);
  const bool stereo = (p.flag[e] & kStereo) != 0;
  const int kf = p.e_kf[e], rows = stereo ? 3 : 2;
  const size_t E = (size_t)p.E;
  double A[3][3], B[3][6];
  edge_jacobians(p.cam[kf], p.est[buf][kf], Xc, stereo, A, B);
  const double w = p.w[e], wo = rho1 * w;
  double omega_r[3];  // omega_r = -(omega * e) * rho1
  for (int r = 0; r < 3; r++) omega_r[r] = -(w * err[r]) * rho1;
  int h = 0;
  for (int a = 0; a < 3; a++)
    for (int c = a; c < 3; c++, h++) {
      double s = 0.0;
      for (int r = 0; r < rows; r++) s = s + (A[r][a] * wo) * A[r][c];
      p.HllC[h * E + e] = s;
    }
  for (int a = 0; a < 3; a++) {
    double s = 0.0;
    for (int r = 0; r < rows; r++) s = s + A[r][a] * omega_r[r];
    p.HllC[(6 + a) * E + e] = s;
  }
  if (p.e_opt[e] < 0) return rho0;  // a fixed pose vertex: the point's blocks alone
  h = 0;
  for (int a = 0; a < 6; a++)
    for (int c = a; c < 6; c++, h++) {
      double s = 0.0;
      for (int r = 0; r < rows; r++) s = s + (B[r][a] * wo) * B[r][c];
      p.HppC[h * E + e] = s;
    }
  for (int a = 0; a < 6; a++) {
    double s = 0.0;
    for (int r = 0; r < rows; r++) s = s + B[r][a] * omega_r[r];
    p.HppC[(21 + a) * E + e] = s;
  }
  for (int a = 0; a < 6; a++)
    for (int c = 0; c < 3; c++) {
      double s = 0.0;
      for (int r = 0; r < rows; r++) s = s + (B[r][a] * wo) * A[r][c];
      p.Hpl[(size_t)e * kHpl + (a * 3 + c)] = s;
    }
  return rho0;
}

// std::max(fabs(v), maxDiagonal)
VSG_HD double max_diag(double m, double v) {
  const double d = __builtin_fabs(v);
  return d < m ? m : d;
}

// PHASE gather, one point: Hll / bl serial over its edges.  Returns the largest |diagonal| (0 for an empty list).
VSG_HD double gather_point(const Prob &p, int pt) {
  const size_t E = (size_t)p.E;
  double acc[kHllC];
  for (int k = 0; k < kHllC; k++) acc[k] = 0.0;
  for (int e = p.p_off[pt]; e < p.p_off[pt + 1]; e++)
    for (int k = 0; k < kHllC; k++) acc[k] = acc[k] + p.HllC[k * E + e];
  for (int k = 0; k < kHllC; k++) p.Hll[(size_t)pt * kHllC + k] = acc[k];
  return max_diag(max_diag(max_diag(0.0, acc[0]), acc[3]), acc[5]);
}

// PHASE gather, lane t's part of optimised keyframe i
VSG_HD void gather_kf_partial(const Prob &p, int i, int t, double *acc) {
  const size_t E = (size_t)p.E;
  for (int k = 0; k < kHppC; k++) acc[k] = 0.0;
  for (int j = p.k_off[i] + t; j < p.k_off[i + 1]; j += kThreads) {
    const int e = p.k_edge[j];
    for (int k = 0; k < kHppC; k++) acc[k] = acc[k] + p.HppC[k * E + e];
  }
}
VSG_HD void gather_kf_store(const Prob &p, int i, const double *acc) {
  for (int k = 0; k < kHppC; k++) p.Hpp[(size_t)i * kHppC + k] = acc[k];
  double m = 0.0;
  for (int a = 0, h = 0; a < 6; h += 6 - a, a++) m = max_diag(m, acc[h]);
  p.maxKf[i] = m;
}

// activeRobustChi2 at the head of an iteration, computeLambdaInit on iteration 0 (one lane)
VSG_HD void begin_iteration(const Prob &p, int it) {
  State &S = *p.S;
  double chi = 0.0;
  for (int g = 0; g < p.Ge; g++) chi = chi + p.chiPart[g];
  S.currentChi = S.tempChi = S.iniChi = chi;
  if (it == 0) {
    double m = 0.0;
    for (int i = 0; i < p.Ko; i++) m = max_diag(m, p.maxKf[i]);
    for (int g = 0; g < p.Gp; g++) m = max_diag(m, p.maxPart[g]);
    S.lambda = 1e-5 * m, S.ni = 2.0, S.n_bad = 0, S.chi2_initial = chi;
  }
  S.rho = 0.0, S.qmax = 0, S.trial_open = 1;
}

// (Hll + lambda I)^-1 of a point as a 3x3 inverse by cofactors; symmetric by construction
VSG_HD void point_dinv(const double *H, double lambda, double D[3][3]) {
  const double a = H[0] + lambda, b = H[1], c = H[2], d = H[3] + lambda, e = H[4], f = H[5] + lambda;
  const double c00 = d * f - e * e, c01 = c * e - b * f, c02 = b * e - c * d;
  const double c11 = a * f - c * c, c12 = b * c - a * e, c22 = a * d - b * b;
  const double det = (a * c00 + b * c01) + c * c02, inv = 1.0 / det;
  D[0][0] = c00 * inv, D[0][1] = D[1][0] = c01 * inv, D[0][2] = D[2][0] = c02 * inv;
  D[1][1] = c11 * inv, D[1][2] = D[2][1] = c12 * inv, D[2][2] = c22 * inv;
}

// PHASE trial 1, one edge of an optimised keyframe: B Dinv and (B Dinv) bl
VSG_HD void trial_edge(const Prob &p, int e, double lambda) {
  if (p.e_opt[e] < 0) return;
  const size_t E = (size_t)p.E;
  const double *H = p.Hll + (size_t)p.e_pt[e] * kHllC;
  double D[3][3];
  point_dinv(H, lambda, D);
  for (int a = 0; a < 6; a++) {
    const double *B = p.Hpl + (size_t)e * kHpl + a * 3;
    const double b0 = B[0], b1 = B[1], b2 = B[2];
    double r[3];
    for (int c = 0; c < 3; c++) r[c] = (b0 * D[0][c] + b1 * D[1][c]) + b2 * D[2][c];
    for (int c = 0; c < 3; c++) p.BDinv[(size_t)e * kHpl + (a * 3 + c)] = r[c];
    p.c[a * E + e] = (r[0] * H[6] + r[1] * H[7]) + r[2] * H[8];
  }
}

// row r of (B Dinv) of edge ea times row c of B of edge eb
VSG_HD double schur_term(const Prob &p, int ea, int eb, int r, int c) {
  const double *W = p.BDinv + (size_t)ea * kHpl + r * 3, *B = p.Hpl + (size_t)eb * kHpl + c * 3;
  return (W[0] * B[0] + W[1] * B[1]) + W[2] * B[2];
}

// PHASE trial 2, entry (r, c) of Schur block blk = (i <= j): Hpp's entry on the diagonal blocks, lambda on the diagonal,
// minus the block's pairs in point order.  Stored at the LOWER mirror (6 j + c, 6 i + r); of a diagonal block the
// entries r <= c alone are stored.
VSG_HD void schur_entry(const Prob &p, int blk, int r, int c, double lambda) {
  const int i = p.b_i[blk], j = p.b_j[blk];
  if (i == j && r > c) return;
  double s = 0.0;
  if (i == j) {
    int h = 0;
    for (int a = 0; a < r; a++) h += 6 - a;
    s = p.Hpp[(size_t)i * kHppC + h + (c - r)];
    if (r == c) s = s + lambda;
  }
  // four pairs' loads are issued before the first is needed; the terms are still subtracted one by one in list order
  const int k1 = p.b_off[blk + 1];
  int k = p.b_off[blk];
  for (; k + 4 <= k1; k += 4) {
    double t[4];
    for (int u = 0; u < 4; u++) t[u] = schur_term(p, p.pair_a[k + u], p.pair_b[k + u], r, c);
    for (int u = 0; u < 4; u++) s = s - t[u];
  }
  for (; k < k1; k++) s = s - schur_term(p, p.pair_a[k], p.pair_b[k], r, c);
  p.M[(size_t)(6 * j + c) * p.n + (6 * i + r)] = s;
}
// lane t's part of bschur of optimised keyframe i: the sum of (B Dinv) bl over its edges
VSG_HD void bschur_partial(const Prob &p, int i, int t, double *acc) {
  const size_t E = (size_t)p.E;
  for (int k = 0; k < kC; k++) acc[k] = 0.0;
  for (int j = p.k_off[i] + t; j < p.k_off[i + 1]; j += kThreads) {
    const int e = p.k_edge[j];
    for (int k = 0; k < kC; k++) acc[k] = acc[k] + p.c[k * E + e];
  }
}
VSG_HD void bschur_store(const Prob &p, int i, const double *acc) {
  for (int k = 0; k < kC; k++) p.bs[6 * i + k] = p.Hpp[(size_t)i * kHppC + 21 + k] - acc[k];
}

// PHASE trial 4, one point: xl = Dinv (bl - B^T xp), the trial estimate, and its part of computeScale
VSG_HD double backsub_point(const Prob &p, int pt, int cur, double lambda) {
  const double *Xc = p.X[cur] + 3 * (size_t)pt;
  double *Xn = p.X[cur ^ 1] + 3 * (size_t)pt;
  if (p.p_off[pt] == p.p_off[pt + 1]) {  // not a vertex
    Xn[0] = Xc[0], Xn[1] = Xc[1], Xn[2] = Xc[2];
    return 0.0;
  }
  const double *H = p.Hll + (size_t)pt * kHllC;
  double r[3] = {H[6], H[7], H[8]};
  for (int e = p.p_off[pt]; e < p.p_off[pt + 1]; e++) {
    const int o = p.e_opt[e];
    if (o < 0) continue;
    const double *x = p.xp + 6 * o;
    for (int c = 0; c < 3; c++) {
      double s = 0.0;
      for (int a = 0; a < 6; a++) s = s + p.Hpl[(size_t)e * kHpl + (a * 3 + c)] * x[a];
      r[c] = r[c] - s;
    }
  }
  double D[3][3], xl[3];
  point_dinv(H, lambda, D);
  for (int c = 0; c < 3; c++) xl[c] = (D[c][0] * r[0] + D[c][1] * r[1]) + D[c][2] * r[2];
  for (int c = 0; c < 3; c++) Xn[c] = Xc[c] + xl[c];  // VertexSBAPointXYZ::oplusImpl
  double v = 0.0;
  for (int c = 0; c < 3; c++) v = v + xl[c] * (lambda * xl[c] + H[6 + c]);
  return v;
}
VSG_HD void oplus_kf(const Prob &p, int i, int cur) {
  const int kf = p.opt_kf[i];
  p.est[cur ^ 1][kf] = pose::est_oplus(p.est[cur][kf], p.xp + 6 * i);
}

// PHASE trial 6 (one lane): tempChi, computeScale, rho, accept or reject, the loop's exits
VSG_HD void decide(const Prob &p) {
  State &S = *p.S;
  double tempChi = 0.0;
  for (int g = 0; g < p.Ge; g++) tempChi = tempChi + p.chiPart[g];
  if (!*p.ok2) tempChi = 1.7976931348623157e308;
  S.tempChi = tempChi;
  double scale = 0.0;
  for (int i = 0; i < p.Ko; i++)
    for (int k = 0; k < 6; k++) {
      const double x = p.xp[6 * i + k];
      scale = scale + x * (S.lambda * x + p.Hpp[(size_t)i * kHppC + 21 + k]);
    }
  for (int g = 0; g < p.Gp; g++) scale = scale + p.scalePart[g];
  scale = scale + 1e-3;
  double rho = S.currentChi - tempChi;
  rho = rho / scale;
  if (rho > 0 && tempChi - tempChi == 0.0) {  // g2o_isfinite(tempChi)
    const double q = 2 * rho - 1;
    double alpha = 1.0 - q * q * q;
    alpha = 2.0 / 3.0 < alpha ? 2.0 / 3.0 : alpha;
    const double f = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;
    S.lambda = S.lambda * f, S.ni = 2.0, S.currentChi = tempChi;
    S.cur ^= 1;  // discardTop: the trial estimates are the estimates
  } else {
    S.lambda = S.lambda * S.ni, S.ni = S.ni * 2.0;  // pop: the other buffer is overwritten by the next trial
  }
  S.rho = rho, S.qmax++, S.trials_run++;
  if (rho < 0 && S.qmax < kTrials) return;
  S.trial_open = 0, S.iterations_run++;
  if (S.qmax == kTrials || rho == 0) {
    S.finished = 1, S.stop_reason = kStopTerminate;
    return;
  }
  if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi)
    S.n_bad++;
  else
    S.n_bad = 0;
  if (S.n_bad >= 3) {
    S.finished = 1, S.stop_reason = kStopBad;
    return;
  }
  S.iter++;
  if (S.iter >= p.iterations) S.finished = 1, S.stop_reason = kStopIterations;
}

// PHASE final, one edge: vToErase and the chi2 compared (:2296-2340)
VSG_HD void classify_edge(const Prob &p, int e, int cur, uint8_t *erase, double *chi2_out) {
  const bool stereo = (p.flag[e] & kStereo) != 0;
  const pose::Edge Ed = edge_of(p, e, p.X[cur]);
  const Est &T = p.est[cur][p.e_kf[e]];
  double r[3];
  pose::quat_rotate(T.q, Ed.X, r);
  const bool depth_positive = r[2] + T.t[2] > 0.0;
  const double chi2 = p.chi2[e];
  erase[e] = (chi2 > (stereo ? 7.815 : 5.991) || !depth_positive) ? 1 : 0;
  if (chi2_out) chi2_out[e] = pose::canon(chi2);
}
VSG_HD vsg_pose_se3d pose_out(const Est &T) {
  vsg_pose_se3d o;
  for (int k = 0; k < 4; k++) o.q[k] = pose::canon(T.q[k]);
  for (int k = 0; k < 3; k++) o.t[k] = pose::canon(T.t[k]);
  return o;
}
// the out of a keyframe that is no vertex of the system (fixed, or without an edge): its input, widened
VSG_HD vsg_pose_se3d pose_widened(const vsg_pose_se3 &T) {
  vsg_pose_se3d o;
  for (int k = 0; k < 4; k++) o.q[k] = (double)T.q[k];
  for (int k = 0; k < 3; k++) o.t[k] = (double)T.t[k];
  return o;
}

// ---- host only from here: the argument check and the lists the kernels walk (the library and the host core share it)

struct Topology {
  int K = 0, Ko = 0, P = 0, E = 0, n_fixed = 0, n_opt = 0;
  std::vector<int32_t> p_off, e_kf, e_pt, e_opt, e_idx, k_off, k_edge, b_i, b_j, b_off, pair_a, pair_b, opt_kf, opt_of;
};

// Everything vsg_mappoints_local_bundle_adjustment checks that needs no device.  kf_n[k] = features of keyframe k whose
// octave the host can see, octave(k, idx) = that octave, nleft[k] = Nleft.  *ran = 0: VSG_OK and the call returns before
// optimize (:1734, :2277, :2283).  max_opt_kf / need_fixed: the local call's cap and its return without a fixed keyframe
// (:1734); vsg_global_ba.h passes its own cap and no such return.  extra_cnt[k] / extra_edges: edges of keyframe k and in
// all that are not in the lists (vsg_sgraph_ba.h's plane edges): they make a keyframe a vertex and keep :2277 from returning.
template <class OctaveOf>
inline int check_and_build(int n_points, const int32_t *slots, const int32_t *obs_off, const int32_t *obs_kf,
                           const int32_t *obs_idx, int n_kf, const int32_t *kf_n, const int32_t *nleft, OctaveOf octave,
                           const uint8_t *kf_fixed, int capacity, int nlevels, int iterations,
                           const volatile uint8_t *stop_flag, Topology *T, int *ran, int max_opt_kf = kMaxOptKf,
                           bool need_fixed = true, const int32_t *extra_cnt = nullptr, int extra_edges = 0) {
  *ran = 0;
  if (n_points < 0 || n_kf < 0 || nlevels < 1 || nlevels > 16 || iterations < 1 || iterations > 100) return VSG_ERR_INVALID;
  if (n_points == 0) return VSG_OK;
  if (!slots || !obs_off || obs_off[0] != 0) return VSG_ERR_INVALID;
  for (int i = 0; i < n_points; i++)
    if (obs_off[i + 1] < obs_off[i]) return VSG_ERR_INVALID;
  const int E = obs_off[n_points];
  if (E > 0 && (!obs_kf || !obs_idx)) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kf_fixed || !kf_n || !nleft)) return VSG_ERR_INVALID;
  for (int e = 0; e < E; e++) {
    if (obs_kf[e] < 0 || obs_kf[e] >= n_kf) return VSG_ERR_INVALID;
    if (obs_idx[e] < 0 || obs_idx[e] >= kf_n[obs_kf[e]]) return VSG_ERR_INVALID;
    const int o = octave(obs_kf[e], obs_idx[e]);
    if (o < 0 || o >= nlevels) return VSG_ERR_INVALID;
  }
  std::vector<uint64_t> seen(((size_t)capacity + 63) / 64, 0);
  for (int i = 0; i < n_points; i++) {
    const int s = slots[i];
    if (s < 0 || s >= capacity) return VSG_ERR_INVALID;
    const uint64_t bit = (uint64_t)1 << (s & 63);
    if (seen[(size_t)s >> 6] & bit) return VSG_ERR_INVALID;
    seen[(size_t)s >> 6] |= bit;
  }
  for (int k = 0; k < n_kf; k++)
    if (nleft[k] != -1) return VSG_ERR_UNSUPPORTED;
  T->K = n_kf, T->P = n_points, T->E = E, T->n_fixed = T->n_opt = 0;
  for (int k = 0; k < n_kf; k++) (kf_fixed[k] ? T->n_fixed : T->n_opt)++;
  if ((need_fixed && T->n_fixed == 0) || E + extra_edges == 0) return VSG_OK;  // :1734, :2277
  std::vector<int32_t> cnt((size_t)n_kf, 0);
  for (int e = 0; e < E; e++) cnt[(size_t)obs_kf[e]]++;
  for (int k = 0; extra_cnt && k < n_kf; k++) cnt[(size_t)k] += extra_cnt[k];
  T->opt_of.assign((size_t)n_kf, -1), T->opt_kf.clear();
  for (int k = 0; k < n_kf; k++)
    if (!kf_fixed[k] && cnt[(size_t)k] > 0) T->opt_of[(size_t)k] = (int32_t)T->opt_kf.size(), T->opt_kf.push_back(k);
  T->Ko = (int)T->opt_kf.size();
  if (T->Ko == 0 || T->Ko > max_opt_kf) return VSG_ERR_UNSUPPORTED;
  if (stop_flag && *stop_flag) return VSG_OK;  // :2283
  const size_t Es = (size_t)E;
  T->p_off.assign(obs_off, obs_off + n_points + 1), T->e_kf.assign(obs_kf, obs_kf + E), T->e_idx.assign(obs_idx, obs_idx + E), T->e_pt.resize(Es), T->e_opt.resize(Es);
  for (int i = 0; i < n_points; i++)
    for (int e = obs_off[i]; e < obs_off[i + 1]; e++) T->e_pt[(size_t)e] = i;
  T->k_off.assign((size_t)T->Ko + 1, 0);
  for (int e = 0; e < E; e++) {
    const int o = T->opt_of[(size_t)obs_kf[e]];
    T->e_opt[(size_t)e] = o;
    if (o >= 0) T->k_off[(size_t)o + 1]++;
  }
  for (int i = 0; i < T->Ko; i++) T->k_off[(size_t)i + 1] += T->k_off[(size_t)i];
  T->k_edge.resize((size_t)T->k_off[(size_t)T->Ko]);
  {
    std::vector<int32_t> at(T->k_off.begin(), T->k_off.end() - 1);
    for (int e = 0; e < E; e++)
      if (T->e_opt[(size_t)e] >= 0) T->k_edge[(size_t)at[(size_t)T->e_opt[(size_t)e]]++] = e;
  }
  // the Schur blocks (i <= j), every one of them, and their pairs in point order
  const int Ko = T->Ko, nb = Ko * (Ko + 1) / 2;
  auto blk = [Ko](int i, int j) { return i * Ko - i * (i - 1) / 2 + (j - i); };
  T->b_i.resize((size_t)nb), T->b_j.resize((size_t)nb), T->b_off.assign((size_t)nb + 1, 0);
  for (int i = 0; i < Ko; i++)
    for (int j = i; j < Ko; j++) T->b_i[(size_t)blk(i, j)] = i, T->b_j[(size_t)blk(i, j)] = j;
  for (int pass = 0; pass < 2; pass++) {
    std::vector<int32_t> at(T->b_off.begin(), T->b_off.end() - 1);
    for (int pt = 0; pt < n_points; pt++)
      for (int a = obs_off[pt]; a < obs_off[pt + 1]; a++) {
        const int i = T->e_opt[(size_t)a];
        if (i < 0) continue;
        for (int b = obs_off[pt]; b < obs_off[pt + 1]; b++) {
          const int j = T->e_opt[(size_t)b];
          if (j < i) continue;
          const size_t B = (size_t)blk(i, j);
          if (pass == 0)
            T->b_off[B + 1]++;
          else
            T->pair_a[(size_t)at[B]] = a, T->pair_b[(size_t)at[B]] = b, at[B]++;
        }
      }
    if (pass == 0) {
      for (int b = 0; b < nb; b++) T->b_off[(size_t)b + 1] += T->b_off[(size_t)b];
      T->pair_a.resize((size_t)T->b_off[(size_t)nb]), T->pair_b.resize((size_t)T->b_off[(size_t)nb]);
    }
  }
  *ran = 1;
  return VSG_OK;
}

inline void fill_result(vsg_local_ba_result *res, const Topology &T, const State *S) {
  memset(res, 0, sizeof(*res));
  res->ran = S ? 1 : 0;
  res->n_opt_kf = T.n_opt, res->n_fixed_kf = T.n_fixed, res->n_points = T.P, res->n_edges = T.E;
  if (!S) return;
  res->n_mono = S->n_mono, res->n_stereo = S->n_stereo;
  res->iterations_run = S->iterations_run, res->trials_run = S->trials_run, res->stop_reason = S->stop_reason;
  res->lambda = pose::canon(S->lambda), res->chi2_initial = pose::canon(S->chi2_initial), res->chi2_final = pose::canon(S->currentChi);
}

// the reduced solve on the host: (i, j) takes -(L_ik L_jk) D_k in ascending k, as the device's right-looking sweep gives it
inline bool solve_reduced_host(int n, double *M, const double *bs, double *x) {
  bool ok = true;
  std::vector<double> D((size_t)n), y((size_t)n);
  auto A = [&](int i, int j) -> double & { return M[(size_t)i * n + j]; };
  for (int j = 0; j < n; j++) {
    double d = A(j, j);
    for (int k = 0; k < j; k++) d = d - (A(j, k) * A(j, k)) * D[(size_t)k];
    D[(size_t)j] = d;
    if (d <= 0.0) ok = false;
    for (int i = j + 1; i < n; i++) {
      double s = A(i, j);
      for (int k = 0; k < j; k++) s = s - (A(i, k) * A(j, k)) * D[(size_t)k];
      A(i, j) = s / d;
    }
  }
  for (int i = 0; i < n; i++) {
    double s = bs[i];
    for (int k = 0; k < i; k++) s = s - A(i, k) * y[(size_t)k];
    y[(size_t)i] = s;
  }
  for (int i = n - 1; i >= 0; i--) {
    double s = y[(size_t)i] / D[(size_t)i];
    for (int k = n - 1; k > i; k--) s = s - A(k, i) * x[k];
    x[i] = s;
  }
  return ok;
}

// The whole call on the host, phase by phase as vsg_local_ba.hip enqueues them, every sum in the device's tree.
struct HostRun {
  Topology T;
  Prob p;
  State S;
  int32_t ok2 = 1;
  std::vector<Cam> cam;
  std::vector<Est> est[2];
  std::vector<double> X[2], obs, w, chi2, Hpl, HppC, HllC, BDinv, c, Hpp, Hll, M, bs, xp, chiPart, maxPart, maxKf, scalePart;
  std::vector<uint8_t> flag;

  // kx / ky / ur: per EDGE (the observed keypoint's), oct per edge; pos = the points' positions in list order
  void setup(const float *pos, const float *kx, const float *ky, const float *ur, const int32_t *oct, const vsg_pose_se3 *Tcw,
             const uint8_t *fixed, const vsg_ba_camera *kc, const float *sig, int nlevels, int iterations) {
    const size_t E = (size_t)T.E, P = (size_t)T.P, K = (size_t)T.K, Ko = (size_t)T.Ko;
    memset(&S, 0, sizeof(S));
    cam.resize(K), est[0].resize(K), est[1].resize(K);
    for (size_t k = 0; k < K; k++) {
      cam[k] = Cam{(double)kc[k].fx, (double)kc[k].fy, (double)kc[k].cx, (double)kc[k].cy, (double)kc[k].bf};
      est[0][k] = est[1][k] = pose::est_from_pose(Tcw[k].q, Tcw[k].t);  // :1766, :1783
    }
    X[0].resize(3 * P), X[1].resize(3 * P);
    for (size_t i = 0; i < 3 * P; i++) X[0][i] = X[1][i] = (double)pos[i];
    obs.resize(3 * E), w.resize(E), flag.resize(E), chi2.assign(E, 0.0);
    for (size_t e = 0; e < E; e++) {
      const bool stereo = ur[e] >= 0;
      obs[e] = (double)kx[e], obs[E + e] = (double)ky[e], obs[2 * E + e] = stereo ? (double)ur[e] : 0.0;
      const int o = oct[e] & 15;
      w[e] = (double)sig[o < nlevels ? o : nlevels - 1];
      flag[e] = stereo ? kStereo : 0;
      (stereo ? S.n_stereo : S.n_mono)++;
    }
    Hpl.assign(kHpl * E, 0.0), HppC.assign(kHppC * E, 0.0), HllC.assign(kHllC * E, 0.0), BDinv.assign(kHpl * E, 0.0), c.assign(kC * E, 0.0);
    Hpp.assign(kHppC * Ko, 0.0), Hll.assign(kHllC * P, 0.0);
    const size_t n = 6 * Ko;
    M.assign(n * n, 0.0), bs.assign(n, 0.0), xp.assign(n, 0.0);
    const size_t Ge = (E + kThreads - 1) / kThreads, Gp = (P + kThreads - 1) / kThreads;
    chiPart.assign(Ge, 0.0), maxPart.assign(Gp, 0.0), scalePart.assign(Gp, 0.0), maxKf.assign(Ko, 0.0);
    p.K = T.K, p.Ko = T.Ko, p.P = T.P, p.E = T.E, p.n = (int)n, p.nb = (int)T.b_i.size(), p.Ge = (int)Ge, p.Gp = (int)Gp;
    p.iterations = iterations;
    p.p_off = T.p_off.data(), p.e_kf = T.e_kf.data(), p.e_pt = T.e_pt.data(), p.e_opt = T.e_opt.data(), p.k_off = T.k_off.data(), p.k_edge = T.k_edge.data();
    p.b_i = T.b_i.data(), p.b_j = T.b_j.data(), p.b_off = T.b_off.data(), p.pair_a = T.pair_a.data(), p.pair_b = T.pair_b.data();
    p.opt_kf = T.opt_kf.data(), p.cam = cam.data(), p.obs = obs.data(), p.w = w.data(), p.flag = flag.data();
    p.est[0] = est[0].data(), p.est[1] = est[1].data(), p.X[0] = X[0].data(), p.X[1] = X[1].data(), p.chi2 = chi2.data();
    p.Hpl = Hpl.data(), p.HppC = HppC.data(), p.HllC = HllC.data(), p.BDinv = BDinv.data(), p.c = c.data(), p.Hpp = Hpp.data();
    p.Hll = Hll.data(), p.M = M.data(), p.bs = bs.data(), p.xp = xp.data(), p.chiPart = chiPart.data(), p.maxPart = maxPart.data();
    p.maxKf = maxKf.data(), p.scalePart = scalePart.data(), p.ok2 = &ok2, p.S = &S;
  }
  // one value per item of [0, count) in groups of kThreads through the tree (items past count give 0)
  template <class F>
  void grouped(int count, double *part_out, F item) {
    static thread_local double part[kThreads][1];
    for (int g = 0; g * kThreads < count; g++) {
      for (int t = 0; t < kThreads; t++) part[t][0] = g * kThreads + t < count ? item(g * kThreads + t) : 0.0;
      pose::HostTeam::tree<1>(part, 1, &part_out[g]);
    }
  }
  void error_pass(int buf) {
    grouped(p.E, chiPart.data(), [&](int e) {
      double err[3], Xc[3], rho1;
      return edge_cost(p, e, buf, err, Xc, &rho1);
    });
  }
  void run(const volatile uint8_t *stop_flag) {
    for (int it = 0; it < p.iterations; it++) {
      if (!run_iteration(S, it)) break;
      grouped(p.E, chiPart.data(), [&](int e) { return linearise_edge(p, e, S.cur); });
      max_groups();
      for (int i = 0; i < p.Ko; i++) {
        static thread_local double part[kThreads][kHppC];
        double acc[kHppC];
        for (int t = 0; t < kThreads; t++) gather_kf_partial(p, i, t, part[t]);
        pose::HostTeam::tree<kHppC>(part, kHppC, acc);
        gather_kf_store(p, i, acc);
      }
      begin_iteration(p, it);
      for (int q = 0; q < kTrials; q++) {
        if (!run_trial(S, it, q)) break;
        const double lambda = S.lambda;
        const int cur = S.cur;
        for (int e = 0; e < p.E; e++) trial_edge(p, e, lambda);
        for (int b = 0; b < p.nb; b++)
          for (int r = 0; r < 6; r++)
            for (int cc = 0; cc < 6; cc++) schur_entry(p, b, r, cc, lambda);
        for (int i = 0; i < p.Ko; i++) {
          static thread_local double part[kThreads][kC];
          double acc[kC];
          for (int t = 0; t < kThreads; t++) bschur_partial(p, i, t, part[t]);
          pose::HostTeam::tree<kC>(part, kC, acc);
          bschur_store(p, i, acc);
        }
        ok2 = solve_reduced_host(p.n, p.M, p.bs, p.xp) ? 1 : 0;
        grouped(p.P, scalePart.data(), [&](int pt) { return backsub_point(p, pt, cur, lambda); });
        for (int i = 0; i < p.Ko; i++) oplus_kf(p, i, cur);
        error_pass(cur ^ 1);
        decide(p);
      }
      if (!S.finished && stop_flag && *stop_flag) S.finished = 1, S.stop_reason = kStopFlag;
    }
  }
  // the lambda-init maximum of the points, group by group through the tree's visiting order
  void max_groups() {
    for (int g = 0; g < p.Gp; g++) {
      double v[kThreads];
      for (int t = 0; t < kThreads; t++) v[t] = g * kThreads + t < p.P ? gather_point(p, g * kThreads + t) : 0.0;
      maxPart[(size_t)g] = max_tree(v);
    }
  }
  static double max_tree(const double *in) {
    double wave[pose::kWaves];
    for (int wv = 0; wv < pose::kWaves; wv++) {
      double v[pose::kWave], o[pose::kWave];
      for (int l = 0; l < pose::kWave; l++) v[l] = in[wv * pose::kWave + l];
      for (int s = 1; s < pose::kWave; s <<= 1) {
        for (int l = 0; l < pose::kWave; l++) o[l] = max_pair(v[l], v[l ^ s]);
        for (int l = 0; l < pose::kWave; l++) v[l] = o[l];
      }
      wave[wv] = v[0];
    }
    double t = wave[0];
    for (int wv = 1; wv < pose::kWaves; wv++) t = max_pair(t, wave[wv]);
    return t;
  }
  // the outs: erase / chi2 per edge, the poses, the float positions (a point that is not a vertex: its input)
  void outputs(const vsg_pose_se3 *Tcw, const float *pos_in, vsg_pose_se3d *kf_out, float *pos_out, uint8_t *erase, double *chi2_out) {
    for (int e = 0; e < p.E; e++) classify_edge(p, e, S.cur, erase, chi2_out);
    for (int k = 0; k < p.K; k++) kf_out[k] = T.opt_of[(size_t)k] >= 0 ? pose_out(est[S.cur][(size_t)k]) : pose_widened(Tcw[k]);
    for (int i = 0; i < p.P; i++)
      for (int d = 0; d < 3; d++)
        pos_out[3 * i + d] = p.p_off[i] == p.p_off[i + 1] ? pos_in[3 * i + d] : pose::canonf((float)X[S.cur][3 * (size_t)i + d]);
  }
  static double max_pair(double a, double b) { return a < b ? b : a; }
};

}  // namespace lba
}  // namespace vsg
