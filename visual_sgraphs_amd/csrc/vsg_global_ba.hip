// vsg_global_ba.hip -- the visual part of Optimizer::BundleAdjustment (Optimizer.cc:60-287, :500-610) on resident keyframes
// and resident map points: vsg_mappoints_global_bundle_adjustment (include/vsg_orb.h).  The arithmetic is csrc/vsg_local_ba.h
// with the kernel type and the blocked schedule of csrc/vsg_global_ba.h, shared with the host build bit for bit; this file
// adds the kernels that differ from the local call's (k_backsub, k_final) and the enqueue policy; the kernels both calls have in
// common are ONE copy, csrc/vsg_ba_kernels.inc, and the reduced solve's chain is csrc/vsg_ldl_chain.inc, which
// vsg_essential_graph.hip includes too.
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
#include "vsg_frame_int.h"
#include "vsg_global_ba.h"

using namespace vsg;

namespace {

enum { kThreads = lba::kThreads, W = gba::kPanel, TS = gba::kTile, WP = W + 1 };
#include "vsg_ba_kernels.inc"

struct FinalArgs {
  const int32_t *slots;
  float *pos;  // the store's, written when write_store
  const vsg_pose_se3 *Tcw;
  const int32_t *opt_of;
  double *chi2;
  vsg_pose_se3d *kf_out;
  float *pos_out;
  int write_store;
};

#include "vsg_ldl_chain.inc"

// workgroups [0, Gp): one lane per point; [Gp, Gp + Gk): the optimised keyframes' oplus, one lane per keyframe
__global__ __launch_bounds__(kThreads) void k_backsub(lba::Prob p, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, tid = threadIdx.x, cur = p.S->cur;
  if (g >= p.Gp) {
    const int i = (g - p.Gp) * kThreads + tid;
    if (i < p.Ko) lba::oplus_kf(p, i, cur);
    return;
  }
  const int pt = g * kThreads + tid;
  double v = pt < p.P ? lba::backsub_point(p, pt, cur, p.S->lambda) : 0.0;
  block_tree<1, false>(&v, lds);
  if (tid == 0) p.scalePart[g] = v;
}

// the write-back (:500-610): the poses, the positions (into the store when write_store), chi2 per edge
__global__ __launch_bounds__(kThreads) void k_final(lba::Prob p, FinalArgs A) {
  const int i = blockIdx.x * kThreads + threadIdx.x, cur = p.S->cur;
  if (i < p.E) A.chi2[i] = pose::canon(p.chi2[i]);
  if (i < p.K) A.kf_out[i] = A.opt_of[i] >= 0 ? lba::pose_out(p.est[cur][i]) : lba::pose_widened(A.Tcw[i]);
  if (i < p.P) {
    const size_t s = (size_t)A.slots[i];
    const bool vertex = p.p_off[i] != p.p_off[i + 1];
    for (int d = 0; d < 3; d++) {
      const float v = vertex ? pose::canonf((float)p.X[cur][3 * (size_t)i + d]) : A.pos[3 * s + d];
      A.pos_out[3 * (size_t)i + d] = v;
      if (vertex && A.write_store) A.pos[3 * s + d] = v;
    }
  }
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
  if (!store_fields(mp, &F) || n_kf < 0 || !inv_level_sigma2 || !kf_Tcw_out || !included || !res) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kfs || !kf_Tcw || !kf_fixed || !kf_cam)) return VSG_ERR_INVALID;
  for (int k = 0; k < n_kf; k++)
    if (frame_check(kfs[k]) != VSG_OK || kfs[k]->device != F.device) return VSG_ERR_INVALID;
  std::vector<int32_t> kf_n((size_t)n_kf), nleft((size_t)n_kf);
  for (int k = 0; k < n_kf; k++) {
    const size_t have = kfs[k]->h_kps.size();
    kf_n[(size_t)k] = (int32_t)((size_t)kfs[k]->n < have ? (size_t)kfs[k]->n : have);
    nleft[(size_t)k] = kfs[k]->nleft;
  }
  lba::Topology T;
  int ran = 0;
  int rc = gba::check_and_build(
      n_points, slots, obs_off, obs_kf, obs_idx, n_kf, kf_n.data(), nleft.data(),
      [&](int k, int i) { return (int)kfs[k]->h_kps[(size_t)i].octave; }, kf_fixed, F.capacity, nlevels, iterations, robust,
      write_store, world_pos_out, stop_flag, &T, &ran);
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
  const SetupArgs &SA = G.SA;
  uint8_t *hp = G.hp, *dp = G.dp, *dv = G.dv;
  const size_t in_bytes = G.in_bytes, Ge = G.Ge, Gp = G.Gp, oChi2 = G.out_off[0], oKfOut = G.out_off[1], oPosOut = G.out_off[2];
  lba::State *mirror = G.mirror, *mirror_dev = G.mirror_dev;
  Solve sv;
  sv.n = (int)n, sv.M = p.M, sv.bs = p.bs, sv.xp = p.xp, sv.D = (double *)(dv + G.dev_off[0]), sv.y = (double *)(dv + G.dev_off[1]);
  sv.acc = (double *)(dv + G.dev_off[2]), sv.ok2 = p.ok2, sv.S = p.S;
  FinalArgs FA;
  FA.slots = SA.slots, FA.pos = F.pos, FA.Tcw = G.Tcw_dev, FA.opt_of = G.opt_of_dev;
  FA.chi2 = (double *)(dp + oChi2), FA.kf_out = (vsg_pose_se3d *)(dp + oKfOut), FA.pos_out = (float *)(dp + oPosOut);
  FA.write_store = write_store;
  const gba::Kernel kernel{robust};

  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, c->stream));
  // from here on an error waits for the stream before it returns: the arenas belong to the next call
  hipStream_t st = c->stream;
  const dim3 B(kThreads);
  const unsigned gAll = G.gAll;
  const int Gs = G.Gs;
  hipLaunchKernelGGL(k_setup, dim3(gAll), B, 0, st, p, SA);
  bool failed = false, stopped = false;
  for (int it = 0; it < iterations && !failed; it++) {
    hipLaunchKernelGGL(k_linearise<gba::Kernel>, dim3((unsigned)Ge), B, 0, st, p, it, kernel);
    hipLaunchKernelGGL(k_gather, dim3((unsigned)(Gp + Ko)), B, 0, st, p, it);
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, p, it, mirror_dev);
    bool closed = false;
    // one trial is enqueued, then the host looks (the local call's measured policy: every further slot is a chain of
    // launches that return at once in the common case of one trial per iteration)
    for (int q = 0; q < lba::kTrials && !closed && !failed; q++) {
      hipLaunchKernelGGL(k_trial_edges, dim3((unsigned)Ge), B, 0, st, p, it, q);
      hipLaunchKernelGGL(k_schur, dim3((unsigned)(Gs + (int)Ko)), B, 0, st, p, it, q, Gs);
      enqueue_solve(st, sv, it, q);
      hipLaunchKernelGGL(k_backsub, dim3((unsigned)(Gp + Gk)), B, 0, st, p, it, q);
      hipLaunchKernelGGL(k_error<gba::Kernel>, dim3((unsigned)Ge), B, 0, st, p, it, q, kernel);
      hipLaunchKernelGGL(k_decide, dim3(1), dim3(1), 0, st, p, it, q, mirror_dev);
      // the look: the record in the pinned arena as the last one-lane step left it
      if (hipGetLastError() != hipSuccess || hipStreamSynchronize(st) != hipSuccess) failed = true;
      closed = failed || mirror->finished || !(mirror->iter == it && mirror->trial_open);
    }
    if (failed || mirror->finished) break;
    if (stop_flag && *stop_flag) {  // terminate() between iterations (sparse_optimizer.cpp:423)
      stopped = true;
      break;
    }
  }
  if (!failed) {
    hipLaunchKernelGGL(k_final, dim3(gAll), B, 0, st, p, FA);
    if (hipGetLastError() != hipSuccess) failed = true;
  }
  if (hipStreamSynchronize(st) != hipSuccess || failed) return VSG_ERR_HIP;
  lba::State Sfin = *mirror;
  if (stopped) Sfin.finished = 1, Sfin.stop_reason = lba::kStopFlag;
  gba::fill_result(res, T, &Sfin);
  if (chi2) memcpy(chi2, hp + oChi2, E * 8);
  memcpy(kf_Tcw_out, hp + oKfOut, K * sizeof(vsg_pose_se3d));
  if (world_pos_out) memcpy(world_pos_out, hp + oPosOut, P * 12);
  return VSG_OK;
}

}  // extern "C"
