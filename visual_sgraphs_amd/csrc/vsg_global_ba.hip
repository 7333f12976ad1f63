// vsg_global_ba.hip -- the visual part of Optimizer::BundleAdjustment (Optimizer.cc:60-287, :500-610) on resident keyframes
// and resident map points: vsg_mappoints_global_bundle_adjustment (include/vsg_orb.h).  The arithmetic is csrc/vsg_local_ba.h
// with the kernel type and the blocked schedule of csrc/vsg_global_ba.h, shared with the host build bit for bit; this file
// adds the final kernel and the entry points.  The kernels both calls have in common are ONE copy, csrc/vsg_ba_kernels.inc;
// the reduced solve's chain is csrc/vsg_ldl_chain.inc, which vsg_essential_graph.hip includes too; the enqueue policy is
// csrc/vsg_lm_driver.h.
//
// KERNEL BOUNDARIES ON THE CALLING THREAD'S STREAM ARE THE ONLY SYNCHRONISATION BETWEEN WORKGROUPS, as in vsg_local_ba.hip:
// no grid-wide barrier, no cooperative launch, no flag between workgroups, nothing spins.  The Levenberg controller
// (lba::State) lives in device memory, is written by the one-lane steps k_begin and k_decide alone, and is read first by
// every kernel, the solver's included, which returns at once when its iteration or trial is not to run.
//
// The phases are those of the local call (k_linearise, k_gather, k_begin; per trial k_trial_edges, k_schur, THE REDUCED SOLVE,
// k_backsub, k_error, k_decide) with the same reduction trees, so that a problem both calls accept gives the same bits.  The
// serial walks over the per-workgroup partials in k_begin and k_decide are kept (a map of 500000 observations has 1954
// partials); the keyframes' oplus is spread over as many workgroups as the keyframes need.
//
// THE REDUCED SOLVE is a blocked right-looking LDL^T over the lower triangle in global memory and two blocked substitutions,
// one code path for every n from 1 to 6 gba::kMaxOptKf.  Per panel of gba::kPanel columns three launches: k_ldl_diag (one
// workgroup factors the diagonal block in LDS), k_ldl_panel (workgroups of gba::kTile rows finish the panel's multipliers
// below it), k_ldl_trail (one workgroup per kTile x kTile tile of the trailing lower triangle stages the panel's L rows of its
// row tile and of its column tile and the panel's D in LDS, reads them once, and gives every element its kPanel updates in
// ascending k from registers).  Then one launch per panel forward (k_fwd) and one per panel backward (k_bwd); in both every
// workgroup solves the panel's small triangle for itself in LDS and then updates its rows of the vector, and workgroup 0
// alone writes the panel's results, to an array nobody reads in that launch.  The number of launches depends on n alone.
// Two multiplies and one add per update, in double, on the vector ALU: no MFMA, no fused multiply-add (-ffp-contract=off).
// All stores are plain vector stores; the two edge counts are integer atomics.
#include <cstring>

#include "../../include/vsg_orb_debug_global_ba.h"
#include "vsg_block_tree.h"
#include "vsg_frame_int.h"
#include "vsg_global_ba.h"
#include "vsg_lm_driver.h"

using namespace vsg;

namespace {

enum { kThreads = lba::kThreads, W = gba::kPanel, TS = gba::kTile, WP = W + 1 };
#include "vsg_ba_kernels.inc"

struct FinalArgs {
  WriteBack wb;
  double *chi2;
  int write_store;
};

#include "vsg_ldl_chain.inc"

// the write-back (:500-610): the poses, the positions (into the store when write_store), chi2 per edge
__global__ __launch_bounds__(kThreads) void k_final(lba::Prob p, FinalArgs A) {
  const int i = blockIdx.x * kThreads + threadIdx.x, cur = p.S->cur;
  if (i < p.E) A.chi2[i] = pose::canon(p.chi2[i]);
  write_back(p, A.wb, i, cur, A.write_store != 0);
}

// a controller record under which every kernel of the chain runs as trial (0, 0): the debug hook's
__global__ void k_debug_open(lba::State *S) {
  lba::State z;
  memset(&z, 0, sizeof(z));
  z.trial_open = 1;
  *S = z;
}

}  // namespace

extern "C" {

int vsg_debug_ba_solver_geometry(int *panel, int *tile) {
  if (!panel || !tile) return VSG_ERR_INVALID;
  *panel = gba::kPanel, *tile = gba::kTile;
  return VSG_OK;
}

int vsg_debug_ba_reduced_solve(int n, const double *M, const double *b, double *x, int *ok) {
  if (n < 1 || n > 6 * gba::kMaxOptKf || !M || !b || !x || !ok) return VSG_ERR_INVALID;
  int device = 0, rc = VSG_OK;
  if (hipGetDevice(&device) != hipSuccess) return VSG_ERR_NO_DEVICE;
  ThreadCtx *c = thread_ctx(device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n;
  Stage in;
  const size_t oM = in.add(N * N * 8), oB = in.add(N * 8), oOk = in.add(4);
  const size_t in_bytes = in.total;
  Stage out = in;
  const size_t oX = out.add(N * 8), oOkOut = out.add(4);
  Stage dev = in;
  const size_t dXp = dev.add(N * 8), dD = dev.add(N * 8), dY = dev.add(N * 8), dAcc = dev.add(N * 8), dS = dev.add(sizeof(lba::State));
  rc = ctx_reserve(c, out.total, dev.total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dv = c->d_buf;
  memcpy(hp + oM, M, N * N * 8), memcpy(hp + oB, b, N * 8);
  *(int32_t *)(hp + oOk) = 1;
  Solve s;
  s.n = n, s.M = (double *)(dv + oM), s.bs = (const double *)(dv + oB), s.xp = (double *)(dv + dXp), s.D = (double *)(dv + dD);
  s.y = (double *)(dv + dY), s.acc = (double *)(dv + dAcc), s.ok2 = (int32_t *)(dv + oOk), s.S = (const lba::State *)(dv + dS);
  hipStream_t st = c->stream;
  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, st));
  hipLaunchKernelGGL(k_debug_open, dim3(1), dim3(1), 0, st, (lba::State *)(dv + dS));
  enqueue_solve(st, s, 0, 0);
  bool failed = hipGetLastError() != hipSuccess;
  if (!failed && hipMemcpyAsync(hp + oX, dv + dXp, N * 8, hipMemcpyDeviceToHost, st) != hipSuccess) failed = true;
  if (!failed && hipMemcpyAsync(hp + oOkOut, dv + oOk, 4, hipMemcpyDeviceToHost, st) != hipSuccess) failed = true;
  if (hipStreamSynchronize(st) != hipSuccess || failed) return VSG_ERR_HIP;
  memcpy(x, hp + oX, N * 8);
  *ok = *(const int32_t *)(hp + oOkOut);
  return VSG_OK;
}

int vsg_mappoints_global_bundle_adjustment(vsg_mappoints *mp, int n_points, const int32_t *slots, const int32_t *obs_off,
                                           const int32_t *obs_kf, const int32_t *obs_idx, int n_kf, vsg_frame *const *kfs,
                                           const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam,
                                           const float *inv_level_sigma2, int nlevels, int iterations, int robust,
                                           int write_store, const volatile uint8_t *stop_flag, vsg_pose_se3d *kf_Tcw_out,
                                           float *world_pos_out, uint8_t *included, double *chi2, vsg_global_ba_result *res) {
  StoreFields F;
  KfLists L;
  int rc = ba_prologue(mp, n_kf, kfs, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, kf_Tcw_out && included && res, &F, &L);
  if (rc != VSG_OK) return rc;
  lba::Topology T;
  int ran = 0;
  rc = gba::check_and_build(n_points, slots, obs_off, obs_kf, obs_idx, n_kf, L.kf_n.data(), L.nleft.data(), L.octave(), kf_fixed,
                            F.capacity, nlevels, iterations, robust, write_store, world_pos_out, stop_flag, &T, &ran);
  if (rc != VSG_OK) return rc;
  if (!ran) {
    if (n_points == 0) T.n_fixed = T.n_opt = 0;
    if (n_points > 0) gba::fill_included(included, n_points, obs_off);
    gba::fill_result(res, T, nullptr);
    return VSG_OK;
  }
  // everything the kernels index has been bounded; nothing has been enqueued
  ThreadCtx *c = thread_ctx(F.device, &rc);
  if (!c) return rc;
  const size_t E = (size_t)T.E, P = (size_t)T.P, K = (size_t)T.K, Ko = (size_t)T.Ko, n = 6 * Ko, Gk = (Ko + kThreads - 1) / kThreads;
  // the pinned arena behind the lists: chi2, the poses, the positions as the kernels write them back; the device arena
  // behind the local call's scratch: the pivots and the two work vectors of the reduced solve
  const size_t outs[3] = {E * 8, K * sizeof(vsg_pose_se3d), P * 12}, devs[3] = {n * 8, n * 8, n * 8};
  Staged G;
  rc = stage_problem(c, F, T, slots, kfs, kf_Tcw, kf_cam, inv_level_sigma2, nlevels, iterations, outs, 3, devs, 3, &G);
  if (rc != VSG_OK) return rc;
  gba::fill_included(included, n_points, obs_off);  // the first out written: no refusal and no failed reservation is left
  const lba::Prob &p = G.p;
  uint8_t *hp = G.hp, *dp = G.dp, *dv = G.dv;
  const size_t Ge = G.Ge, Gp = G.Gp, oChi2 = G.out_off[0], oKfOut = G.out_off[1], oPosOut = G.out_off[2];
  lba::State *mirror_dev = G.mirror_dev;
  Solve sv;
  sv.n = (int)n, sv.M = p.M, sv.bs = p.bs, sv.xp = p.xp, sv.D = (double *)(dv + G.dev_off[0]), sv.y = (double *)(dv + G.dev_off[1]);
  sv.acc = (double *)(dv + G.dev_off[2]), sv.ok2 = p.ok2, sv.S = p.S;
  FinalArgs FA;
  FA.wb = G.wb, FA.wb.kf_out = (vsg_pose_se3d *)(dp + oKfOut), FA.wb.pos_out = (float *)(dp + oPosOut);
  FA.chi2 = (double *)(dp + oChi2), FA.write_store = write_store;
  const gba::Kernel kernel{robust};

  TRY_HIP(hipMemcpyAsync(dv, hp, G.in_bytes, hipMemcpyHostToDevice, c->stream));
  hipStream_t st = c->stream;
  const dim3 B(kThreads);
  const int Gs = G.Gs;
  hipLaunchKernelGGL(k_setup, dim3(G.gAll), B, 0, st, p, G.SA);
  lba::State Sfin;
  const bool done = lm::run(
      st, G.mirror, iterations, lm::kTrialSlots, stop_flag,
      [&](int it) {
        hipLaunchKernelGGL(k_linearise<gba::Kernel>, dim3((unsigned)Ge), B, 0, st, p, it, kernel);
        hipLaunchKernelGGL(k_gather, dim3((unsigned)(Gp + Ko)), B, 0, st, p, it);
        hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, p, it, mirror_dev);
      },
      [&](int it, int q) {
        hipLaunchKernelGGL(k_trial_edges, dim3((unsigned)Ge), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_schur, dim3((unsigned)(Gs + (int)Ko)), B, 0, st, p, it, q, Gs);
        enqueue_solve(st, sv, it, q);
        hipLaunchKernelGGL(k_backsub, dim3((unsigned)(Gp + Gk)), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_error<gba::Kernel>, dim3((unsigned)Ge), B, 0, st, p, it, q, kernel);
        hipLaunchKernelGGL(k_decide, dim3(1), dim3(1), 0, st, p, it, q, mirror_dev);
      },
      [&] { hipLaunchKernelGGL(k_final, dim3(G.gAll), B, 0, st, p, FA); },
      &Sfin);
  if (!done) return VSG_ERR_HIP;
  gba::fill_result(res, T, &Sfin);
  if (chi2) memcpy(chi2, hp + oChi2, E * 8);
  memcpy(kf_Tcw_out, hp + oKfOut, K * sizeof(vsg_pose_se3d));
  if (world_pos_out) memcpy(world_pos_out, hp + oPosOut, P * 12);
  return VSG_OK;
}

}  // extern "C"
