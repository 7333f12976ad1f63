// vsg_essential_graph.h -- Optimizer::OptimizeEssentialGraph, first overload (Optimizer.cc:2456-2734), host and device from
// one source: the pose graph over Sim3 vertices that LoopClosing::CorrectLoop runs at LoopClosing.cc:1150, and the point
// correction behind it (:2704-2731; the same arithmetic at LoopClosing.cc:1060-1064).  The kernels of
// vsg_essential_graph.hip run the per-item functions below over the whole chip; tests/_egcore and the latency probe's
// caller-side path compile the same functions for the host and replay every sum in the same order (HostRun).  The pattern
// is vsg_sim3_opt.h's, whose Sim3 algebra (sim3_exp, sim3_mul, sim3_inverse, sim3_oplus, exp_sim3) is used as it is.
//
// Everything is double, as g2o has it; both builds use -ffp-contract=off.  What is restated, and from where:
//   * g2o::Sim3::log() (Thirdparty/g2o/g2o/types/sim3.h:141-216): toRotationMatrix, d, deltaR and skew (se3_ops.hpp), all four
//     branches on fabs(sigma) < 1e-5 and d > 1 - 1e-5, and W.lu().solve(t) as Eigen's PartialPivLU at 3 x 3, WITH its row
//     swaps (lu3_solve).  log is written out here (dlog: fdlibm's e_log.c; the CPU test measures it against libm), acos is
//     mlpnp::dacos, sin / cos are pose::sincos_pose;
//   * EdgeSim3::computeError (types_seven_dof_expmap.h:107-115): (C * v1 * v2^-1).log(), information = the 7 x 7 identity
//     multiplied out as Eigen does, chi2 = e . (I e);
//   * the NUMERIC Jacobian of BaseBinaryEdge::linearizeOplus (base_binary_edge.hpp:131-205) for BOTH vertices: column d is
//     (1 / (2 delta)) (e(+delta e_d) - e(-delta e_d)), delta = 1e-9, the perturbation through oplusImpl
//     (types_seven_dof_expmap.h:62-71), so with fix_scale column 6 is exactly zero; a fixed vertex gets no block.  The 14
//     factors exp(+-delta e_d) do not depend on the estimate: they are computed once per call (perturbation);
//   * constructQuadraticForm without a robust kernel (base_binary_edge.hpp:55-86): H_ii, H_ij, H_jj, b_i, b_j per edge;
//   * the system H + lambda I over the non-fixed vertices with at least one edge, in ascending vertex order (g2o drops a
//     vertex without an edge: it keeps its input), every sum over edges in ascending edge index, which is g2o's insertion
//     order, the caller's list order;
//   * OptimizationAlgorithmLevenberg with setUserLambdaInit(1e-16) and optimize(20) (:2469, :2684): computeLambdaInit returns
//     the user value; computeScale reads x AFTER oplusImpl zeroed its [6] entries; trials, qmax == 10, rho and _nBad as
//     optimization_algorithm_levenberg.cpp:61-199 has them.  The controller's record is lba::State, so that the dense solve's
//     chain (vsg_ldl_chain.inc) gates on it as it is; the controller itself (begin_iteration, decide) is this routine's own;
//   * the measurements (:2536-2551, :2568-2598, :2610-2623, :2641-2656): Sji = Sjw * Swi; a "loop" edge takes both sides
//     from vScw, a "normal" edge takes each side from NonCorrectedSim3 where the keyframe has an entry, else from vScw;
//   * the point correction (:2723-2728): float(correctedSwr.map(Srw.map(double(float pos)))).
// NOT here: the merge overload (:2736 ff.), OptimizeEssentialGraph4DoF, the inertial edges (:2662-2679).
//
// THE SOLVE is dense: an LDL^T without pivoting over all 7 n_opt rows (the reference: Eigen's sparse SimplicialLDLT behind
// an AMD ordering; equal to rounding on a positive-definite system).  A pivot <= 0 gives ok2 = false and tempChi = DBL_MAX,
// as a failed Cholesky does.  The schedule is gba::solve_reduced_blocked_host's, bit-equal to the device chain.
//
// No floating-point atomics.  Every loop bound is a compile-time constant or a count the host validated.
#pragma once
#include <stdint.h>
#include <string.h>

#include <vector>

#include "../../include/vsg_orb.h"
#include "vsg_global_ba.h"
#include "vsg_mlpnp.h"
#include "vsg_sim3_opt.h"

namespace vsg {
namespace eg {

using sim3opt::Sim3;

// kMaxOptKf: 7 * 438 = 3066 <= 3072 rows, the range the chain is tested over
enum { kThreads = lba::kThreads, kDim = 7, kMaxOptKf = 438, kPert = 2 * kDim, kSlots = 2 * kPert + 1 };
// one edge's blocks, 119 doubles at [119 e]: H_ii upper triangle row by row | H_ij 7 x 7 row-major | H_jj upper | b_i | b_j
enum { kTri = 28, oHii = 0, oHij = kTri, oHjj = kTri + 49, oBi = 2 * kTri + 49, oBj = oBi + kDim, kBlock = oBj + kDim };
// a contribution to a block of the system: 4 edge + kind
enum { kKindII = 0, kKindJJ = 1, kKindIJ = 2, kKindJI = 3 };

// ---- log for Sim3::log()'s `sigma = std::log(s)`: fdlibm's e_log.c for a normal positive x; anything else (zero, negative,
// subnormal, infinite, NaN) gives NaN: the scale is validated > 0 on entry, and a NaN error rejects the trial.
VSG_HD double dlog(double x) {
  const double ln2_hi = 6.93147180369123816490e-01, ln2_lo = 1.90821492927058770002e-10, Lg1 = 6.666666666666735130e-01,
               Lg2 = 3.999999999940941908e-01, Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
               Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01, Lg7 = 1.479819860511658591e-01;
  const uint64_t bits = mlpnp::d2u(x);
  int32_t hx = (int32_t)(bits >> 32);
  if (hx < 0x00100000 || hx >= 0x7ff00000) return __builtin_nan("");
  int32_t k = (hx >> 20) - 1023;
  hx &= 0x000fffff;
  int32_t i = (hx + 0x95f64) & 0x100000;
  x = mlpnp::u2d(((uint64_t)(uint32_t)(hx | (i ^ 0x3ff00000)) << 32) | (bits & 0xffffffffull));  // x or x / 2
  k += (i >> 20);
  const double f = x - 1.0, dk = (double)k;
  if ((0x000fffff & (2 + hx)) < 3) {  // |f| < 2^-20
    if (f == 0.0) return k == 0 ? 0.0 : dk * ln2_hi + dk * ln2_lo;
    const double R = f * f * (0.5 - 0.33333333333333333 * f);
    return k == 0 ? f - R : dk * ln2_hi - ((R - dk * ln2_lo) - f);
  }
  const double s = f / (2.0 + f), z = s * s, w = z * z;
  i = hx - 0x6147a;
  const int32_t j = 0x6b851 - hx;
  const double t1 = w * (Lg2 + w * (Lg4 + w * Lg6)), t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)));
  i |= j;
  const double R = t2 + t1;
  if (i > 0) {
    const double hfsq = 0.5 * f * f;
    return k == 0 ? f - (hfsq - s * (hfsq + R)) : dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f);
  }
  return k == 0 ? f - s * (f - R) : dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f);
}

// ---- W.lu().solve(t): Eigen's PartialPivLU at 3 x 3.  Per column the row of the largest |entry| at or below the diagonal
// (the first of equals) comes up; a zero pivot column is left as it is (its division then gives inf or NaN in the
// substitution, as Eigen's does).  Rows are exchanged by value, never by index: no array is indexed by a variable.
VSG_HD void lu3_swap(bool c, double *a, double *b) {
  const double x = *a, y = *b;
  *a = c ? y : x, *b = c ? x : y;
}
VSG_HD void lu3_solve(const double W[3][3], const double *t, double *x) {
  double a00 = W[0][0], a01 = W[0][1], a02 = W[0][2], a10 = W[1][0], a11 = W[1][1], a12 = W[1][2], a20 = W[2][0], a21 = W[2][1],
         a22 = W[2][2], b0 = t[0], b1 = t[1], b2 = t[2];
  {  // column 0
    const double m0 = __builtin_fabs(a00), m1 = __builtin_fabs(a10), m2 = __builtin_fabs(a20);
    const bool s1 = m1 > m0, s2 = m2 > (s1 ? m1 : m0);
    const bool up1 = s1 && !s2;
    lu3_swap(up1, &a00, &a10), lu3_swap(up1, &a01, &a11), lu3_swap(up1, &a02, &a12), lu3_swap(up1, &b0, &b1);
    lu3_swap(s2, &a00, &a20), lu3_swap(s2, &a01, &a21), lu3_swap(s2, &a02, &a22), lu3_swap(s2, &b0, &b2);
    if (a00 != 0.0) a10 = a10 / a00, a20 = a20 / a00;
    a11 = a11 - a10 * a01, a12 = a12 - a10 * a02;
    a21 = a21 - a20 * a01, a22 = a22 - a20 * a02;
  }
  {  // column 1
    const bool s = __builtin_fabs(a21) > __builtin_fabs(a11);
    lu3_swap(s, &a10, &a20), lu3_swap(s, &a11, &a21), lu3_swap(s, &a12, &a22), lu3_swap(s, &b1, &b2);
    if (a11 != 0.0) a21 = a21 / a11;
    a22 = a22 - a21 * a12;
  }
  // L c = P t (unit lower), U x = c
  const double c0 = b0, c1 = b1 - a10 * c0, c2 = (b2 - a20 * c0) - a21 * c1;
  const double x2 = c2 / a22, x1 = ((c1 - a12 * x2)) / a11, x0 = ((c0 - a01 * x1) - a02 * x2) / a00;
  x[0] = x0, x[1] = x1, x[2] = x2;
}

// ---- g2o::Sim3::log(): res = [omega, upsilon, sigma]
VSG_HD void sim3_log(const Sim3 &S, double *res) {
  const double s = S.s, sigma = dlog(s), eps = 0.00001;
  double R[3][3];
  lba::quat_to_matrix(S.q, R);
  const double d = 0.5 * (((R[0][0] + R[1][1]) + R[2][2]) - 1);
  const double dR[3] = {R[2][1] - R[1][2], R[0][2] - R[2][0], R[1][0] - R[0][1]};  // deltaR
  const bool small_sigma = __builtin_fabs(sigma) < eps, near = d > 1 - eps;
  double f = 0.5, theta = 0.0, sn = 0.0, cs = 1.0;
  if (!near) {
    theta = mlpnp::dacos(d);
    f = theta / (2 * sqrt(1 - d * d));
    pose::sincos_pose(theta, &sn, &cs);
  }
  const double om[3] = {f * dR[0], f * dR[1], f * dR[2]};
  double A, B, C;
  if (small_sigma) {
    C = 1;
    if (near) {
      A = 1. / 2.;
      B = 1. / 6.;
    } else {
      const double theta2 = theta * theta;
      A = (1 - cs) / (theta2);
      B = (theta - sn) / (theta2 * theta);
    }
  } else {
    C = (s - 1) / sigma;
    if (near) {
      const double sigma2 = sigma * sigma;
      A = ((sigma - 1) * s + 1) / (sigma2);
      B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
    } else {
      const double theta2 = theta * theta, a = s * sn, b = s * cs, c = theta2 + sigma * sigma;
      A = (a * sigma + (1 - b) * theta) / (theta * c);
      B = (C - ((b - 1) * sigma + a * theta) / (c)) * 1. / (theta2);
    }
  }
  // W = A * Omega + B * Omega * Omega + C * I, Omega = skew(omega): (B * Omega) times Omega, summed in k order
  const double O[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
  double W[3][3];
  VSG_S3O_UNROLL
  for (int i = 0; i < 3; i++)
    VSG_S3O_UNROLL
    for (int j = 0; j < 3; j++) {
      const double P = ((B * O[i][0]) * O[0][j] + (B * O[i][1]) * O[1][j]) + (B * O[i][2]) * O[2][j];
      W[i][j] = (A * O[i][j] + P) + C * (i == j ? 1.0 : 0.0);
    }
  lu3_solve(W, S.t, res + 3);
  res[0] = om[0], res[1] = om[1], res[2] = om[2], res[6] = sigma;
}

// EdgeSim3::computeError: (C * v1 * v2^-1).log()
VSG_HD void edge_error(const Sim3 &C, const Sim3 &v1, const Sim3 &v2, double *e) {
  sim3_log(sim3opt::sim3_mul(sim3opt::sim3_mul(C, v1), sim3opt::sim3_inverse(v2)), e);
}
// chi2() = e . (I e), the identity multiplied out with its zeros
VSG_HD double edge_chi2(const double *e) {
  double c = 0.0;
  VSG_S3O_UNROLL
  for (int k = 0; k < kDim; k++) {
    double ie = 0.0;
    VSG_S3O_UNROLL
    for (int m = 0; m < kDim; m++) ie = ie + (k == m ? 1.0 : 0.0) * e[m];
    c = c + e[k] * ie;
  }
  return c;
}

// factor k = 2 d + (0: +delta, 1: -delta) of linearizeOplus: Sim3(update) after oplusImpl's `if (_fix_scale) update[6] = 0`
VSG_HD Sim3 perturbation(int k, bool fix_scale) {
  const double delta = 1e-9;
  double u[kDim];
  VSG_S3O_UNROLL
  for (int d = 0; d < kDim; d++) u[d] = d == (k >> 1) ? ((k & 1) ? -delta : delta) : 0.0;
  if (fix_scale) u[6] = 0;
  return sim3opt::sim3_exp(u);
}

// The measurement of one edge (vertex 0 = i, vertex 1 = j): Sji = Sjw * Swi
VSG_HD Sim3 side_of(const vsg_sim3d *Scw, const vsg_sim3d *nonc, const uint8_t *has_nonc, int k, bool loop) {
  return sim3opt::sim3_of((!loop && has_nonc[k]) ? nonc[k] : Scw[k]);
}
VSG_HD Sim3 measurement(const vsg_sim3d *Scw, const vsg_sim3d *nonc, const uint8_t *has_nonc, int i, int j, bool loop) {
  return sim3opt::sim3_mul(side_of(Scw, nonc, has_nonc, j, loop), sim3opt::sim3_inverse(side_of(Scw, nonc, has_nonc, i, loop)));
}

// The point correction: Sto_inv.map(Sfrom.map(double(pos))) narrowed to float
VSG_HD void correct_point(const Sim3 &Sfrom, const Sim3 &Sto_inv, const float *pos, float *out) {
  const double x[3] = {(double)pos[0], (double)pos[1], (double)pos[2]};
  double y[3], z[3];
  sim3opt::sim3_map(Sfrom, x, y);
  sim3opt::sim3_map(Sto_inv, y, z);
  out[0] = pose::canonf((float)z[0]), out[1] = pose::canonf((float)z[1]), out[2] = pose::canonf((float)z[2]);
}

// What the phases index.  Lists are built and bounded by the host (Topology below).
struct Prob {
  int32_t K, Ko, E, n, nb, Ge, iterations, fix_scale;
  const int32_t *e_i, *e_j, *e_oi, *e_oj;  // [E] vertex 0, vertex 1, their index among the optimised vertices (-1: no block)
  const uint8_t *e_loop;                   // [E]
  const int32_t *blk_a, *blk_b, *blk_off, *blk_ent;  // block (a >= b) of the system and its contributions, edges ascending
  const int32_t *v_off, *v_ent;            // [Ko + 1]: optimised vertex a's incident edges ascending, 2 edge + side
  const int32_t *opt_kf;                   // [Ko] keyframe of optimised index a
  const vsg_sim3d *Scw, *nonc;             // [K] the caller's
  const uint8_t *has_nonc;                 // [K]
  Sim3 *meas;                              // [E]
  Sim3 *est[2];                            // [K] each: current = est[S->cur]
  Sim3 *pert;                              // [kPert]
  double *blocks, *chi2;                   // [kBlock E], [E] as the last error pass left it
  double *M, *b, *xp;                      // [n n] row-major (lower triangle used), [n], [n]
  double *chiPart;                         // [Ge]
  int32_t *ok2;
  lba::State *S;
};

// PHASE linearise, slot s of edge e at estimate buffer buf: s < 14 perturbs vertex 0 by factor s, 14 <= s < 28 vertex 1 by
// factor s - 14, s == 28 is the error itself
VSG_HD void slot_error(const Prob &p, int e, int s, int buf, double *err) {
  Sim3 vi = p.est[buf][p.e_i[e]], vj = p.est[buf][p.e_j[e]];
  if (s < kPert)
    vi = sim3opt::sim3_mul(p.pert[s], vi);
  else if (s < 2 * kPert)
    vj = sim3opt::sim3_mul(p.pert[s - kPert], vj);
  edge_error(p.meas[e], vi, vj, err);
}
// column d of a vertex's Jacobian from its two slots' errors
VSG_HD double jacobian_entry(double ep, double em) { return (1.0 / (2 * 1e-9)) * (ep - em); }

// omega_r = -omega * e and AtO = J^T * omega, the identity multiplied out
VSG_HD double omega_r_at(const double *e, int k) {
  double s = 0.0;
  VSG_S3O_UNROLL
  for (int m = 0; m < kDim; m++) s = s + (-(k == m ? 1.0 : 0.0)) * e[m];
  return s;
}
// J is [row][column] with a row stride of ld doubles
VSG_HD double ato_at(const double *J, int ld, int a, int k) {
  double s = 0.0;
  VSG_S3O_UNROLL
  for (int m = 0; m < kDim; m++) s = s + J[m * ld + a] * (m == k ? 1.0 : 0.0);
  return s;
}
// entry x of kBlock of one edge's quadratic form: Ji / Jj = the two Jacobians, e = the error
VSG_HD double block_entry(const double *Ji, const double *Jj, int ld, const double *e, int x) {
  double s = 0.0;
  if (x >= oBi) {  // b_i / b_j: J^T omega_r
    const double *J = x >= oBj ? Jj : Ji;
    const int a = x >= oBj ? x - oBj : x - oBi;
    for (int k = 0; k < kDim; k++) s = s + J[k * ld + a] * omega_r_at(e, k);
    return s;
  }
  const double *L = Ji, *Rm = Ji;
  int a, c;
  if (x >= oHij && x < oHjj) {
    Rm = Jj;
    a = (x - oHij) / kDim, c = (x - oHij) % kDim;
  } else {
    int t = x;
    if (x >= oHjj) L = Rm = Jj, t = x - oHjj;
    a = 0;
    while (t >= kDim - a) t -= kDim - a, a++;
    c = a + t;
  }
  for (int k = 0; k < kDim; k++) s = s + ato_at(L, ld, a, k) * Rm[k * ld + c];
  return s;
}
// whether entry x of edge e is written: a vertex that is fixed (or has no block) gets none
VSG_HD bool block_entry_live(int oi, int oj, int x) {
  if (x >= oBj) return oj >= 0;
  if (x >= oBi) return oi >= 0;
  if (x >= oHjj) return oj >= 0;
  if (x >= oHij) return oi >= 0 && oj >= 0;
  return oi >= 0;
}

// PHASE gather: row r of b, serial over the vertex's incident edges ascending
VSG_HD double gather_b(const Prob &p, int r) {
  const int a = r / kDim, k = r % kDim;
  double s = 0.0;
  for (int x = p.v_off[a]; x < p.v_off[a + 1]; x++) {
    const int ent = p.v_ent[x];
    s = s + p.blocks[(size_t)(ent >> 1) * kBlock + ((ent & 1) ? oBj : oBi) + k];
  }
  return s;
}

VSG_HD int tri_index(int r, int c) {  // (r <= c) of a 7 x 7 upper triangle stored row by row
  return r * kDim - r * (r - 1) / 2 + (c - r);
}

// PHASE assemble, entry (r, c) of block blk = (a >= b) of the lower triangle of H + lambda I; of a diagonal block the
// entries c <= r alone.  A block without a contribution is written as zeros: the factorisation destroys the matrix.
VSG_HD void assemble_entry(const Prob &p, int blk, int r, int c, double lambda) {
  const int a = p.blk_a[blk], b = p.blk_b[blk];
  if (a == b && c > r) return;
  double s = 0.0;
  for (int x = p.blk_off[blk]; x < p.blk_off[blk + 1]; x++) {
    const int ent = p.blk_ent[x], kind = ent & 3;
    const double *B = p.blocks + (size_t)(ent >> 2) * kBlock;
    double v;
    if (kind == kKindII)
      v = B[oHii + tri_index(c, r)];
    else if (kind == kKindJJ)
      v = B[oHjj + tri_index(c, r)];
    else if (kind == kKindIJ)
      v = B[oHij + r * kDim + c];  // vertex 0 is a (the rows)
    else
      v = B[oHij + c * kDim + r];  // vertex 0 is b (the columns): the transposed block
    s = s + v;
  }
  if (a == b && r == c) s = s + lambda;
  p.M[(size_t)(kDim * a + r) * p.n + (kDim * b + c)] = s;
}

// PHASE oplus, optimised vertex a: oplusImpl into the other buffer; x[6] is zeroed IN xp when fix_scale
VSG_HD void oplus_vertex(const Prob &p, int a, int cur) {
  const int kf = p.opt_kf[a];
  p.est[cur ^ 1][kf] = sim3opt::sim3_oplus(p.est[cur][kf], p.xp + kDim * a, p.fix_scale != 0);
}

// computeError + chi2 of edge e at buffer buf; stores chi2[e]
VSG_HD double edge_cost(const Prob &p, int e, int buf) {
  double err[kDim];
  slot_error(p, e, 2 * kPert, buf, err);
  const double c = edge_chi2(err);
  p.chi2[e] = c;
  return c;
}

// activeChi2 at the head of an iteration; computeLambdaInit returns the user value (one lane)
VSG_HD void begin_iteration(const Prob &p, int it) {
  lba::State &S = *p.S;
  double chi = 0.0;
  for (int g = 0; g < p.Ge; g++) chi = chi + p.chiPart[g];
  S.currentChi = S.tempChi = S.iniChi = chi;
  if (it == 0) S.lambda = 1e-16, S.ni = 2.0, S.n_bad = 0, S.chi2_initial = chi;
  S.rho = 0.0, S.qmax = 0, S.trial_open = 1;
}

// one lane: tempChi, computeScale, rho, accept or reject, the loop's exits (no stop flag in this routine)
VSG_HD void decide(const Prob &p) {
  lba::State &S = *p.S;
  double tempChi = 0.0;
  for (int g = 0; g < p.Ge; g++) tempChi = tempChi + p.chiPart[g];
  if (!*p.ok2) tempChi = 1.7976931348623157e308;
  S.tempChi = tempChi;
  double scale = 0.0;
  for (int j = 0; j < p.n; j++) scale = scale + p.xp[j] * (S.lambda * p.xp[j] + p.b[j]);
  scale = scale + 1e-3;
  double rho = S.currentChi - tempChi;
  rho = rho / scale;
  if (rho > 0 && tempChi - tempChi == 0.0) {  // g2o_isfinite(tempChi)
    const double q = 2 * rho - 1;
    double alpha = 1.0 - q * q * q;
    alpha = 2.0 / 3.0 < alpha ? 2.0 / 3.0 : alpha;
    const double f = 1.0 / 3.0 < alpha ? alpha : 1.0 / 3.0;
    S.lambda = S.lambda * f, S.ni = 2.0, S.currentChi = tempChi;
    S.cur ^= 1;  // discardTop
  } else {
    S.lambda = S.lambda * S.ni, S.ni = S.ni * 2.0;  // pop
  }
  S.rho = rho, S.qmax++, S.trials_run++;
  if (rho < 0 && S.qmax < lba::kTrials) return;
  S.trial_open = 0, S.iterations_run++;
  if (S.qmax == lba::kTrials || rho == 0) {
    S.finished = 1, S.stop_reason = lba::kStopTerminate;
    return;
  }
  if ((S.iniChi - S.currentChi) * 1e3 < S.iniChi)
    S.n_bad++;
  else
    S.n_bad = 0;
  if (S.n_bad >= 3) {
    S.finished = 1, S.stop_reason = lba::kStopBad;
    return;
  }
  S.iter++;
  if (S.iter >= p.iterations) S.finished = 1, S.stop_reason = lba::kStopIterations;
}

// ---- host only from here

struct Topology {
  int K = 0, Ko = 0, E = 0, P = 0, n_fixed = 0;
  std::vector<int32_t> e_i, e_j, e_oi, e_oj, blk_a, blk_b, blk_off, blk_ent, v_off, v_ent, opt_kf, opt_of;
  std::vector<uint8_t> e_loop;
};

inline bool sim3_ok(const vsg_sim3d &s) {
  for (int k = 0; k < 4; k++)
    if (!(s.q[k] - s.q[k] == 0.0)) return false;
  for (int k = 0; k < 3; k++)
    if (!(s.t[k] - s.t[k] == 0.0)) return false;
  return s.s - s.s == 0.0 && s.s > 0.0;
}

// a list of store slots with the points' reference index: every slot in [0, capacity) and listed once, every ref in [0, n_ref)
inline bool check_points(int n_points, const int32_t *slots, const int32_t *point_ref, int capacity, int n_ref) {
  if (n_points == 0) return true;
  if (!slots || !point_ref) return false;
  std::vector<uint64_t> seen(((size_t)capacity + 63) / 64, 0);
  for (int i = 0; i < n_points; i++) {
    const int s = slots[i];
    if (s < 0 || s >= capacity || point_ref[i] < 0 || point_ref[i] >= n_ref) return false;
    const uint64_t bit = (uint64_t)1 << (s & 63);
    if (seen[(size_t)s >> 6] & bit) return false;
    seen[(size_t)s >> 6] |= bit;
  }
  return true;
}

// Everything vsg_mappoints_optimize_essential_graph checks that needs no device, and the lists the kernels walk.  capacity
// < 0: the call has no store (legal with n_points == 0 alone).  *ran = 0 with VSG_OK: nothing to optimise (no edge, or no
// edge at a vertex that is not fixed).
inline int check_and_build(int n_kf, const vsg_sim3d *kf_Scw, const vsg_sim3d *kf_nonc, const uint8_t *kf_has_nonc,
                           const uint8_t *kf_fixed, int n_edges, const int32_t *edge_i, const int32_t *edge_j,
                           const uint8_t *edge_loop, int fix_scale, int iterations, int n_points, const int32_t *slots,
                           const int32_t *point_ref, int capacity, const void *kf_out, const void *res, Topology *T, int *ran) {
  *ran = 0;
  if (n_kf < 0 || n_edges < 0 || n_points < 0 || iterations < 1 || iterations > 100 || (fix_scale != 0 && fix_scale != 1))
    return VSG_ERR_INVALID;
  if (!kf_out || !res) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kf_Scw || !kf_has_nonc || !kf_fixed)) return VSG_ERR_INVALID;
  if (n_edges > 0 && (!edge_i || !edge_j || !edge_loop)) return VSG_ERR_INVALID;
  if (n_edges > (1 << 28)) return VSG_ERR_UNSUPPORTED;
  if (n_points > 0 && capacity < 0) return VSG_ERR_INVALID;
  for (int k = 0; k < n_kf; k++) {
    if (!sim3_ok(kf_Scw[k])) return VSG_ERR_INVALID;
    if (kf_has_nonc[k] && (!kf_nonc || !sim3_ok(kf_nonc[k]))) return VSG_ERR_INVALID;
  }
  for (int e = 0; e < n_edges; e++)
    if (edge_i[e] < 0 || edge_i[e] >= n_kf || edge_j[e] < 0 || edge_j[e] >= n_kf || edge_i[e] == edge_j[e]) return VSG_ERR_INVALID;
  if (!check_points(n_points, slots, point_ref, capacity < 0 ? 0 : capacity, n_kf)) return VSG_ERR_INVALID;
  T->K = n_kf, T->E = n_edges, T->P = n_points, T->n_fixed = 0, T->Ko = 0;
  std::vector<int32_t> cnt((size_t)n_kf, 0);
  for (int e = 0; e < n_edges; e++) cnt[(size_t)edge_i[e]]++, cnt[(size_t)edge_j[e]]++;
  T->opt_of.assign((size_t)n_kf, -1), T->opt_kf.clear();
  for (int k = 0; k < n_kf; k++) {
    if (kf_fixed[k]) T->n_fixed++;
    if (!kf_fixed[k] && cnt[(size_t)k] > 0) T->opt_of[(size_t)k] = (int32_t)T->opt_kf.size(), T->opt_kf.push_back(k);
  }
  T->Ko = (int)T->opt_kf.size();
  if (T->Ko > kMaxOptKf) return VSG_ERR_UNSUPPORTED;
  if (n_edges == 0 || T->Ko == 0) return VSG_OK;
  const size_t E = (size_t)n_edges;
  const int Ko = T->Ko, nb = Ko * (Ko + 1) / 2;
  T->e_i.assign(edge_i, edge_i + E), T->e_j.assign(edge_j, edge_j + E), T->e_loop.resize(E), T->e_oi.resize(E), T->e_oj.resize(E);
  for (size_t e = 0; e < E; e++)
    T->e_loop[e] = edge_loop[e] ? 1 : 0, T->e_oi[e] = T->opt_of[(size_t)edge_i[e]], T->e_oj[e] = T->opt_of[(size_t)edge_j[e]];
  auto blk = [](int a, int b) { return a * (a + 1) / 2 + b; };  // a >= b
  T->blk_a.resize((size_t)nb), T->blk_b.resize((size_t)nb), T->blk_off.assign((size_t)nb + 1, 0), T->v_off.assign((size_t)Ko + 1, 0);
  for (int a = 0; a < Ko; a++)
    for (int b = 0; b <= a; b++) T->blk_a[(size_t)blk(a, b)] = a, T->blk_b[(size_t)blk(a, b)] = b;
  for (int pass = 0; pass < 2; pass++) {
    std::vector<int32_t> at(T->blk_off.begin(), T->blk_off.end() - 1), vat(T->v_off.begin(), T->v_off.end() - 1);
    auto add = [&](int a, int b, int e, int kind) {
      const size_t B = (size_t)blk(a, b);
      if (pass == 0)
        T->blk_off[B + 1]++;
      else
        T->blk_ent[(size_t)at[B]++] = 4 * e + kind;
    };
    auto addv = [&](int a, int e, int side) {
      if (pass == 0)
        T->v_off[(size_t)a + 1]++;
      else
        T->v_ent[(size_t)vat[(size_t)a]++] = 2 * e + side;
    };
    for (int e = 0; e < n_edges; e++) {
      const int oi = T->e_oi[(size_t)e], oj = T->e_oj[(size_t)e];
      if (oi >= 0) add(oi, oi, e, kKindII), addv(oi, e, 0);
      if (oj >= 0) add(oj, oj, e, kKindJJ), addv(oj, e, 1);
      if (oi >= 0 && oj >= 0) {
        if (oi > oj)
          add(oi, oj, e, kKindIJ);
        else
          add(oj, oi, e, kKindJI);
      }
    }
    if (pass == 0) {
      for (int b = 0; b < nb; b++) T->blk_off[(size_t)b + 1] += T->blk_off[(size_t)b];
      for (int a = 0; a < Ko; a++) T->v_off[(size_t)a + 1] += T->v_off[(size_t)a];
      T->blk_ent.resize((size_t)T->blk_off[(size_t)nb]), T->v_ent.resize((size_t)T->v_off[(size_t)Ko]);
    }
  }
  *ran = 1;
  return VSG_OK;
}

inline void fill_result(vsg_essential_graph_result *res, const Topology &T, const lba::State *S) {
  memset(res, 0, sizeof(*res));
  res->ran = S ? 1 : 0;
  res->n_opt_kf = T.Ko, res->n_fixed_kf = T.n_fixed, res->n_kf = T.K, res->n_edges = T.E, res->n_points = T.P;
  if (!S) return;
  res->iterations_run = S->iterations_run, res->trials_run = S->trials_run, res->stop_reason = S->stop_reason;
  res->lambda = pose::canon(S->lambda), res->chi2_initial = pose::canon(S->chi2_initial), res->chi2_final = pose::canon(S->currentChi);
}

// The whole call on the host, phase by phase as vsg_essential_graph.hip enqueues them, every sum in the device's order.
struct HostRun {
  Topology T;
  Prob p;
  lba::State S;
  int32_t ok2 = 1;
  std::vector<Sim3> meas, est[2], pert;
  std::vector<double> blocks, chi2, M, b, xp, chiPart;
  std::vector<uint8_t> accepted;  // one flag per trial, in order (the tests compare the decisions)

  void setup(const vsg_sim3d *Scw, const vsg_sim3d *nonc, const uint8_t *has_nonc, int fix_scale, int iterations) {
    const size_t E = (size_t)T.E, K = (size_t)T.K, n = (size_t)kDim * (size_t)T.Ko, Ge = (E + kThreads - 1) / kThreads;
    memset(&S, 0, sizeof(S));
    memset(&p, 0, sizeof(p));
    meas.resize(E), est[0].resize(K), est[1].resize(K), pert.resize(kPert);
    for (size_t k = 0; k < K; k++) est[0][k] = est[1][k] = sim3opt::sim3_of(Scw[k]);  // setEstimate takes the input as it is
    for (int k = 0; k < kPert; k++) pert[(size_t)k] = perturbation(k, fix_scale != 0);
    for (size_t e = 0; e < E; e++) meas[e] = measurement(Scw, nonc, has_nonc, T.e_i[e], T.e_j[e], T.e_loop[e] != 0);
    blocks.assign(kBlock * E, 0.0), chi2.assign(E, 0.0), M.assign(n * n, 0.0), b.assign(n, 0.0), xp.assign(n, 0.0), chiPart.assign(Ge, 0.0);
    p.K = T.K, p.Ko = T.Ko, p.E = T.E, p.n = (int)n, p.nb = (int)T.blk_a.size(), p.Ge = (int)Ge, p.iterations = iterations;
    p.fix_scale = fix_scale;
    p.e_i = T.e_i.data(), p.e_j = T.e_j.data(), p.e_oi = T.e_oi.data(), p.e_oj = T.e_oj.data(), p.e_loop = T.e_loop.data();
    p.blk_a = T.blk_a.data(), p.blk_b = T.blk_b.data(), p.blk_off = T.blk_off.data(), p.blk_ent = T.blk_ent.data();
    p.v_off = T.v_off.data(), p.v_ent = T.v_ent.data(), p.opt_kf = T.opt_kf.data(), p.Scw = Scw, p.nonc = nonc, p.has_nonc = has_nonc;
    p.meas = meas.data(), p.est[0] = est[0].data(), p.est[1] = est[1].data(), p.pert = pert.data(), p.blocks = blocks.data();
    p.chi2 = chi2.data(), p.M = M.data(), p.b = b.data(), p.xp = xp.data(), p.chiPart = chiPart.data(), p.ok2 = &ok2, p.S = &S;
  }
  // chi2[e] of every edge in groups of kThreads through the tree (items past E give 0)
  void chi_groups() {
    static thread_local double part[kThreads][1];
    for (int g = 0; g < p.Ge; g++) {
      for (int t = 0; t < kThreads; t++) part[t][0] = g * kThreads + t < p.E ? chi2[(size_t)(g * kThreads + t)] : 0.0;
      pose::HostTeam::tree<1>(part, 1, &chiPart[(size_t)g]);
    }
  }
  void linearise_edge(int e, int buf) {
    double err[kSlots][kDim], J[2][kDim][kDim];
    for (int s = 0; s < kSlots; s++) slot_error(p, e, s, buf, err[s]);
    for (int v = 0; v < 2; v++)
      for (int d = 0; d < kDim; d++)
        for (int r = 0; r < kDim; r++) J[v][r][d] = jacobian_entry(err[v * kPert + 2 * d][r], err[v * kPert + 2 * d + 1][r]);
    chi2[(size_t)e] = edge_chi2(err[2 * kPert]);
    for (int x = 0; x < kBlock; x++)
      if (block_entry_live(p.e_oi[e], p.e_oj[e], x))
        blocks[(size_t)e * kBlock + x] = block_entry(&J[0][0][0], &J[1][0][0], kDim, err[2 * kPert], x);
  }
  void run() {
    for (int it = 0; it < p.iterations; it++) {
      if (!lba::run_iteration(S, it)) break;
      for (int e = 0; e < p.E; e++) linearise_edge(e, S.cur);
      chi_groups();
      for (int r = 0; r < p.n; r++) b[(size_t)r] = gather_b(p, r);
      begin_iteration(p, it);
      for (int q = 0; q < lba::kTrials; q++) {
        if (!lba::run_trial(S, it, q)) break;
        const int cur = S.cur;
        for (int blk = 0; blk < p.nb; blk++)
          for (int r = 0; r < kDim; r++)
            for (int c = 0; c < kDim; c++) assemble_entry(p, blk, r, c, S.lambda);
        ok2 = gba::solve_reduced_blocked_host(p.n, p.M, p.b, p.xp) ? 1 : 0;
        for (int a = 0; a < p.Ko; a++) oplus_vertex(p, a, cur);
        for (int e = 0; e < p.E; e++) edge_cost(p, e, cur ^ 1);
        chi_groups();
        decide(p);
        accepted.push_back(S.cur != cur ? 1 : 0);
      }
    }
  }
  // the outs: the estimates, chi2 per edge at them (computeActiveErrors after optimize, :2685; may be NULL), and the points
  void outputs(const vsg_sim3d *Scw, vsg_sim3d *kf_out, double *chi2_out) {
    for (int k = 0; k < p.K; k++) kf_out[k] = T.opt_of[(size_t)k] >= 0 ? sim3opt::sim3d_canon(est[S.cur][(size_t)k]) : Scw[k];
    if (chi2_out)
      for (int e = 0; e < p.E; e++) chi2_out[e] = pose::canon(edge_cost(p, e, S.cur));
  }
  void correct(const vsg_sim3d *Scw, int n_points, const int32_t *point_ref, const float *pos_in, float *pos_out) {
    for (int i = 0; i < n_points; i++) {
      const int r = point_ref[i];
      correct_point(sim3opt::sim3_of(Scw[r]), sim3opt::sim3_inverse(est[S.cur][(size_t)r]), pos_in + 3 * (size_t)i, pos_out + 3 * (size_t)i);
    }
  }
};

}  // namespace eg
}  // namespace vsg
