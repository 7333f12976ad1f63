// vsg_local_ba.hip -- the visual part of Optimizer::LocalBundleAdjustment (Optimizer.cc:1454-2454) on resident keyframes
// and resident map points: vsg_mappoints_local_bundle_adjustment (include/vsg_orb.h).  The arithmetic is csrc/vsg_local_ba.h,
// shared with the host build bit for bit.  The kernels around its per-item functions, the reduced solve's sweep among
// them, are csrc/vsg_ba_kernels.inc, the reduction tree on the wavefronts is csrc/vsg_block_tree.h and the enqueue policy
// csrc/vsg_lm_driver.h, each ONE copy for every call that has them; this file adds the classification and the entry point.
//
// KERNEL BOUNDARIES ON THE CALLING THREAD'S STREAM ARE THE ONLY SYNCHRONISATION BETWEEN WORKGROUPS.  There is no grid-wide
// barrier, no cooperative launch, no flag between workgroups and nothing spins.  The Levenberg controller (lba::State:
// lambda, ni, nBad, currentChi, qmax, the iteration, the current estimate buffer, the open / finished flags) lives in device
// memory, is written by the one-lane steps k_begin and k_decide alone, and is read first by every phase kernel, which
// returns at once when its iteration or trial is not to run: the result does not depend on how many trial slots the host
// enqueued ahead nor on when it looks.  k_begin and k_decide mirror the record into the pinned arena for the host's look.
//
// Per iteration: k_linearise (one lane per edge: error, Huber weight, Jacobians, the edge's own blocks, the chi2 partials),
// k_gather (one lane per point: Hll / bl; one workgroup per optimised keyframe: Hpp / bp), k_begin.  Per trial:
// k_trial_edges (B Dinv and B Dinv bl per edge), k_schur (one lane per entry of a Schur block walking the block's pair
// list; one workgroup per keyframe for bschur), k_solve (ONE workgroup, the reduced LDL^T on the matrix in global memory
// and the two triangular solves, one code path for every size up to 768 rows), k_backsub (points, and the keyframes'
// oplus), k_error, k_decide.  push / pop are two estimate buffers and State::cur.
//
// Scratch and lists live in the CALLING THREAD's arenas.  The points' world_pos is written by k_final alone: two threads
// may solve on one store at once only when their point sets are disjoint.  All stores are plain vector stores; the two
// edge counts are integer atomics.
#include <cstring>

#include "../../include/vsg_orb_debug_local_ba.h"
#include "vsg_block_tree.h"
#include "vsg_frame_int.h"
#include "vsg_lm_driver.h"
#include "vsg_local_ba.h"

using namespace vsg;

namespace {

thread_local int t_trial_slots = 0;  // vsg_debug_local_ba_trial_slots: 0 = lm::kTrialSlots

#include "vsg_ba_kernels.inc"

struct FinalArgs {
  WriteBack wb;
  uint8_t *erase;
  double *chi2;
};

// the classification (:2296-2340) and the recovery (:2398-2414)
__global__ __launch_bounds__(lba::kThreads) void k_final(lba::Prob p, FinalArgs A) {
  const int i = blockIdx.x * lba::kThreads + threadIdx.x, cur = p.S->cur;
  if (i < p.E) lba::classify_edge(p, i, cur, A.erase, A.chi2);
  write_back(p, A.wb, i, cur, true);
}

}  // namespace

extern "C" {

int vsg_debug_local_ba_trial_slots(int slots) {
  if (slots < 0 || slots > lba::kTrials) return VSG_ERR_INVALID;
  t_trial_slots = slots;
  return VSG_OK;
}

int vsg_mappoints_local_bundle_adjustment(vsg_mappoints *mp, int n_points, const int32_t *slots, const int32_t *obs_off,
                                          const int32_t *obs_kf, const int32_t *obs_idx, int n_kf, vsg_frame *const *kfs,
                                          const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed, const vsg_ba_camera *kf_cam,
                                          const float *inv_level_sigma2, int nlevels, int iterations,
                                          const volatile uint8_t *stop_flag, vsg_pose_se3d *kf_Tcw_out, float *world_pos_out,
                                          uint8_t *erase, double *chi2, vsg_local_ba_result *res) {
  StoreFields F;
  KfLists L;
  int rc = ba_prologue(mp, n_kf, kfs, kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, kf_Tcw_out && erase && res, &F, &L);
  if (rc != VSG_OK) return rc;
  lba::Topology T;
  int ran = 0;
  rc = lba::check_and_build(n_points, slots, obs_off, obs_kf, obs_idx, n_kf, L.kf_n.data(), L.nleft.data(), L.octave(), kf_fixed,
                            F.capacity, nlevels, iterations, stop_flag, &T, &ran);
  if (rc != VSG_OK) return rc;
  if (!ran) {
    if (n_points == 0) T.n_fixed = T.n_opt = 0;
    lba::fill_result(res, T, nullptr);
    return VSG_OK;
  }
  // everything the kernels index has been bounded; nothing has been enqueued
  ThreadCtx *c = thread_ctx(F.device, &rc);
  if (!c) return rc;
  const size_t E = (size_t)T.E, P = (size_t)T.P, K = (size_t)T.K, Ko = (size_t)T.Ko;
  // the pinned arena behind the lists: erase, chi2, the poses, the positions as the kernels write them back
  const size_t outs[4] = {E, E * 8, K * sizeof(vsg_pose_se3d), P * 12};
  Staged G;
  rc = stage_problem(c, F, T, slots, kfs, kf_Tcw, kf_cam, inv_level_sigma2, nlevels, iterations, outs, 4, nullptr, 0, &G);
  if (rc != VSG_OK) return rc;
  const lba::Prob &p = G.p;
  uint8_t *hp = G.hp, *dp = G.dp;
  const size_t Ge = G.Ge, Gp = G.Gp, oErase = G.out_off[0], oChi2 = G.out_off[1], oKfOut = G.out_off[2], oPosOut = G.out_off[3];
  lba::State *mirror_dev = G.mirror_dev;
  FinalArgs FA;
  FA.wb = G.wb, FA.wb.kf_out = (vsg_pose_se3d *)(dp + oKfOut), FA.wb.pos_out = (float *)(dp + oPosOut);
  FA.erase = dp + oErase, FA.chi2 = (double *)(dp + oChi2);

  TRY_HIP(hipMemcpyAsync(G.dv, hp, G.in_bytes, hipMemcpyHostToDevice, c->stream));
  hipStream_t st = c->stream;
  const dim3 B(lba::kThreads);
  const int Gs = G.Gs;
  hipLaunchKernelGGL(k_setup, dim3(G.gAll), B, 0, st, p, G.SA);
  lba::State Sfin;
  const bool done = lm::run(
      st, G.mirror, iterations, t_trial_slots > 0 ? t_trial_slots : (int)lm::kTrialSlots, stop_flag,
      [&](int it) {
        hipLaunchKernelGGL(k_linearise<lba::HuberLocal>, dim3((unsigned)Ge), B, 0, st, p, it, lba::HuberLocal());
        hipLaunchKernelGGL(k_gather, dim3((unsigned)(Gp + Ko)), B, 0, st, p, it);
        hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, p, it, mirror_dev);
      },
      [&](int it, int q) {
        hipLaunchKernelGGL(k_trial_edges, dim3((unsigned)Ge), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_schur, dim3((unsigned)(Gs + (int)Ko)), B, 0, st, p, it, q, Gs);
        hipLaunchKernelGGL(k_solve<kSolveRows>, dim3(1), dim3(lba::kSolveThreads), 0, st, p, it, q);
        hipLaunchKernelGGL(k_backsub, dim3((unsigned)(Gp + 1)), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_error<lba::HuberLocal>, dim3((unsigned)Ge), B, 0, st, p, it, q, lba::HuberLocal());
        hipLaunchKernelGGL(k_decide, dim3(1), dim3(1), 0, st, p, it, q, mirror_dev);
      },
      [&] { hipLaunchKernelGGL(k_final, dim3(G.gAll), B, 0, st, p, FA); },
      &Sfin);
  if (!done) return VSG_ERR_HIP;
  lba::fill_result(res, T, &Sfin);
  const uint8_t *he = hp + oErase;
  int n_erase = 0;
  for (size_t e = 0; e < E; e++) n_erase += he[e] != 0;
  res->n_erase = n_erase;
  memcpy(erase, he, E);
  if (chi2) memcpy(chi2, hp + oChi2, E * 8);
  memcpy(kf_Tcw_out, hp + oKfOut, K * sizeof(vsg_pose_se3d));
  if (world_pos_out) memcpy(world_pos_out, hp + oPosOut, P * 12);
  return VSG_OK;
}

}  // extern "C"
