// vsg_global_ba.h -- the visual part of Optimizer::BundleAdjustment (Optimizer.cc:60-287, :500-610) behind
// Optimizer::GlobalBundleAdjustemnt (:45-58): every keyframe and every map point of a map, monocular and stereo reprojection
// edges, an OPTIONAL Huber kernel (bRobust), g2o's Levenberg loop over a Schur complement.  Host and device from one source:
// the kernels of vsg_global_ba.hip run the per-item functions of vsg_local_ba.h (the two edges, the Jacobian blocks, the
// gather, the trial, the Schur entry, the back-substitution, the controller, the oplus) with the kernel type below;
// tests/_gbacore and the latency probe compile HostRun for the host, which replays every sum in the same tree.
//
// What differs from the local call, and from where:
//   * the robust kernel is optional (:189, :221) and its monocular delta is sqrt(5.99) (:133), not the sqrt(5.991) of
//     :1847; without it rho = chi2 and the weight is 1 (base_binary_edge.hpp:60-66: the same quadratic form with rho'(e) = 1);
//   * no fixed keyframe is no reason to return, and nothing is classified or recovered after optimize;
//   * the reduced system may have 6 kMaxOptKf = 3072 rows: past one workgroup.  THE REDUCED SOLVE is the blocked schedule
//     below, on the device a chain of kernels (vsg_global_ba.hip), here the same schedule as loops.
//
// THE BLOCKED SCHEDULE.  Panels of kPanel columns, left to right.  Per panel: (1) the diagonal block is factored; (2) the
// rows below it get their multipliers of the panel's columns; (3) every element of the trailing lower triangle takes the
// panel's kPanel updates.  Element (i, j) still receives M_ij - (L_ik L_jk) D_k for ASCENDING k: inside a panel by the loops
// of steps 1 to 3, across panels because panels go left to right; a multiplier is divided by its pivot once, after its last
// update.  y_i receives y_i - L_ik y_k in ascending k (panels left to right, ascending inside), x_i starts as y_i / D_i and
// receives - L_ki x_k in descending k (panels right to left, descending inside).  That is the order of
// lba::solve_reduced_host and of the local call's k_solve: with -ffp-contract=off the three are equal bit for bit, at every
// n, and tests/test_gba_hostmath.py and the GPU test assert it.
#pragma once
#include "vsg_local_ba.h"

namespace vsg {
namespace gba {

// kMaxOptKf: optimised keyframes with edges the call accepts: 3072 rows, a matrix of 3072^2 doubles = 75.5 MB in the calling
// thread's device arena.  kPanel: columns per panel (a multiple of 6: whole keyframes).  kTile: rows and columns of one
// workgroup's tile of the trailing update, and rows per workgroup of step 2.
enum { kMaxOptKf = 512, kPanel = 48, kTile = 64 };

// thHuber2D = sqrt(5.99), thHuber3D = sqrt(7.815) as FLOATs (:133-134), squared after widening by RobustKernelHuber::setDelta
VSG_HD double huber_delta(bool stereo) { return stereo ? (double)2.7955322265625f : (double)2.4474475383758545f; }

// bRobust as a value: what lba::edge_cost / lba::linearise_edge call for rho and rho'
struct Kernel {
  int robust;
  VSG_HD void operator()(double chi2, bool stereo, double *rho0, double *rho1) const {
    if (robust)
      pose::huber(chi2, huber_delta(stereo), rho0, rho1);
    else
      *rho0 = chi2, *rho1 = 1.0;
  }
};

// ---- host only from here

// Everything vsg_mappoints_global_bundle_adjustment checks that needs no device: the local call's checks with this call's
// cap and without the return of :1734, and the three arguments the local call does not have.
template <class OctaveOf>
inline int check_and_build(int n_points, const int32_t *slots, const int32_t *obs_off, const int32_t *obs_kf,
                           const int32_t *obs_idx, int n_kf, const int32_t *kf_n, const int32_t *nleft, OctaveOf octave,
                           const uint8_t *kf_fixed, int capacity, int nlevels, int iterations, int robust, int write_store,
                           const float *world_pos_out, const volatile uint8_t *stop_flag, lba::Topology *T, int *ran) {
  *ran = 0;
  if ((robust != 0 && robust != 1) || (write_store != 0 && write_store != 1)) return VSG_ERR_INVALID;
  if (write_store == 0 && !world_pos_out) return VSG_ERR_INVALID;
  return lba::check_and_build(n_points, slots, obs_off, obs_kf, obs_idx, n_kf, kf_n, nleft, octave, kf_fixed, capacity, nlevels,
                              iterations, stop_flag, T, ran, kMaxOptKf, false);
}

// vbNotIncludedMP (:278-286), negated
inline void fill_included(uint8_t *included, int n_points, const int32_t *obs_off) {
  for (int i = 0; i < n_points; i++) included[i] = obs_off[i + 1] > obs_off[i] ? 1 : 0;
}

inline void fill_result(vsg_global_ba_result *res, const lba::Topology &T, const lba::State *S) {
  memset(res, 0, sizeof(*res));
  res->ran = S ? 1 : 0;
  res->n_opt_kf = T.n_opt, res->n_fixed_kf = T.n_fixed, res->n_points = T.P, res->n_edges = T.E;
  if (!S) return;
  res->n_mono = S->n_mono, res->n_stereo = S->n_stereo;
  res->iterations_run = S->iterations_run, res->trials_run = S->trials_run, res->stop_reason = S->stop_reason;
  res->lambda = pose::canon(S->lambda), res->chi2_initial = pose::canon(S->chi2_initial), res->chi2_final = pose::canon(S->currentChi);
}

// The blocked schedule on the host, step by step as vsg_global_ba.hip enqueues it (D, y and acc are the device's arrays).
inline bool solve_reduced_blocked_host(int n, double *M, const double *bs, double *x) {
  bool ok = true;
  std::vector<double> D((size_t)n), y(bs, bs + n), acc((size_t)n), v((size_t)kPanel);
  auto A = [&](int i, int j) -> double & { return M[(size_t)i * n + j]; };
  for (int c0 = 0; c0 < n; c0 += kPanel) {
    const int w = n - c0 < kPanel ? n - c0 : kPanel, r0 = c0 + w;
    for (int k = 0; k < w; k++) {  // step 1
      const double d = A(c0 + k, c0 + k);
      D[(size_t)(c0 + k)] = d;
      if (d <= 0.0) ok = false;
      for (int i = k + 1; i < w; i++) A(c0 + i, c0 + k) = A(c0 + i, c0 + k) / d;
      for (int i = k + 1; i < w; i++)
        for (int j = k + 1; j <= i; j++) A(c0 + i, c0 + j) = A(c0 + i, c0 + j) - (A(c0 + i, c0 + k) * A(c0 + j, c0 + k)) * d;
    }
    for (int r = r0; r < n; r++)  // step 2
      for (int k = 0; k < w; k++) {
        const double d = D[(size_t)(c0 + k)], l = A(r, c0 + k) / d;
        A(r, c0 + k) = l;
        for (int j = k + 1; j < w; j++) A(r, c0 + j) = A(r, c0 + j) - (l * A(c0 + j, c0 + k)) * d;
      }
    for (int i = r0; i < n; i++)  // step 3
      for (int j = r0; j <= i; j++) {
        double a = A(i, j);
        for (int k = 0; k < w; k++) a = a - (A(i, c0 + k) * A(j, c0 + k)) * D[(size_t)(c0 + k)];
        A(i, j) = a;
      }
  }
  for (int c0 = 0; c0 < n; c0 += kPanel) {  // forward
    const int w = n - c0 < kPanel ? n - c0 : kPanel;
    for (int i = 0; i < w; i++) v[(size_t)i] = y[(size_t)(c0 + i)];
    for (int k = 0; k < w; k++)
      for (int i = k + 1; i < w; i++) v[(size_t)i] = v[(size_t)i] - A(c0 + i, c0 + k) * v[(size_t)k];
    for (int i = c0 + w; i < n; i++) {
      double s = y[(size_t)i];
      for (int k = 0; k < w; k++) s = s - A(i, c0 + k) * v[(size_t)k];
      y[(size_t)i] = s;
    }
    for (int i = 0; i < w; i++) acc[(size_t)(c0 + i)] = v[(size_t)i] / D[(size_t)(c0 + i)];
  }
  for (int c0 = (n - 1) / kPanel * kPanel; c0 >= 0; c0 -= kPanel) {  // backward
    const int w = n - c0 < kPanel ? n - c0 : kPanel;
    for (int i = 0; i < w; i++) v[(size_t)i] = acc[(size_t)(c0 + i)];
    for (int k = w - 1; k > 0; k--)
      for (int i = 0; i < k; i++) v[(size_t)i] = v[(size_t)i] - A(c0 + k, c0 + i) * v[(size_t)k];
    for (int i = 0; i < c0; i++) {
      double s = acc[(size_t)i];
      for (int k = w - 1; k >= 0; k--) s = s - A(c0 + k, i) * v[(size_t)k];
      acc[(size_t)i] = s;
    }
    for (int i = 0; i < w; i++) x[c0 + i] = v[(size_t)i];
  }
  return ok;
}

// The whole call on the host, phase by phase as vsg_global_ba.hip enqueues them: lba::HostRun's set-up, lists and trees
// with this call's kernel and reduced solve, and this call's outs.
struct HostRun : lba::HostRun {
  Kernel kernel{1};
  // the host's look between two iterations, where the device call reads the stop flag: called with the iteration just done,
  // before the flag is read (tests set the flag from here, as another thread would)
  void (*at_look)(void *ctx, int it) = nullptr;
  void *look_ctx = nullptr;

  void error_pass(int buf) {
    grouped(p.E, chiPart.data(), [&](int e) {
      double err[3], Xc[3], rho1;
      return lba::edge_cost(p, e, buf, err, Xc, &rho1, kernel);
    });
  }
  void run(const volatile uint8_t *stop_flag) {
    for (int it = 0; it < p.iterations; it++) {
      if (!lba::run_iteration(S, it)) break;
      grouped(p.E, chiPart.data(), [&](int e) { return lba::linearise_edge(p, e, S.cur, kernel); });
      max_groups();
      for (int i = 0; i < p.Ko; i++) {
        static thread_local double part[lba::kThreads][lba::kHppC];
        double acc[lba::kHppC];
        for (int t = 0; t < lba::kThreads; t++) lba::gather_kf_partial(p, i, t, part[t]);
        pose::HostTeam::tree<lba::kHppC>(part, lba::kHppC, acc);
        lba::gather_kf_store(p, i, acc);
      }
      lba::begin_iteration(p, it);
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
        ok2 = solve_reduced_blocked_host(p.n, p.M, p.bs, p.xp) ? 1 : 0;
        grouped(p.P, scalePart.data(), [&](int pt) { return lba::backsub_point(p, pt, cur, lambda); });
        for (int i = 0; i < p.Ko; i++) lba::oplus_kf(p, i, cur);
        error_pass(cur ^ 1);
        lba::decide(p);
      }
      if (at_look) at_look(look_ctx, it);
      if (!S.finished && stop_flag && *stop_flag) S.finished = 1, S.stop_reason = lba::kStopFlag;
    }
  }
  // the outs: the poses, the float positions (a point that is not a vertex: its input), chi2 per edge (may be NULL)
  void outputs(const vsg_pose_se3 *Tcw, const float *pos_in, vsg_pose_se3d *kf_out, float *pos_out, double *chi2_out) {
    if (chi2_out)
      for (int e = 0; e < p.E; e++) chi2_out[e] = pose::canon(p.chi2[e]);
    for (int k = 0; k < p.K; k++)
      kf_out[k] = T.opt_of[(size_t)k] >= 0 ? lba::pose_out(est[S.cur][(size_t)k]) : lba::pose_widened(Tcw[k]);
    for (int i = 0; i < p.P; i++)
      for (int d = 0; d < 3; d++)
        pos_out[3 * i + d] = p.p_off[i] == p.p_off[i + 1] ? pos_in[3 * i + d] : pose::canonf((float)X[S.cur][3 * (size_t)i + d]);
  }
};

}  // namespace gba
}  // namespace vsg
