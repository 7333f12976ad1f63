// vsg_local_ba.hip -- the visual part of Optimizer::LocalBundleAdjustment (Optimizer.cc:1454-2454) on resident keyframes
// and resident map points: vsg_mappoints_local_bundle_adjustment (include/vsg_orb.h).  The arithmetic is csrc/vsg_local_ba.h,
// shared with the host build bit for bit; this file adds the kernels around its per-item functions, the reduction tree on
// the wavefronts (both in csrc/vsg_ba_kernels.inc where vsg_global_ba.hip has them too), the reduced solve's sweep and the
// enqueue policy.
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
#include "vsg_frame_int.h"
#include "vsg_local_ba.h"

using namespace vsg;

namespace {

// Trial slots enqueued ahead per iteration before the host looks.  MEASURED on the local-BA leg of
// tools/resident_points_probe.py (profiles/local_ba_latency.json), medians of 200 calls with S = 1 / 2 / 10:
//   10 + 10 keyframes, 1500 points: 2559 / 2646 / 3357 us;  20 + 20, 3000: 3970 / 4036 / 4727;  40 + 40, 6000: 10526 /
//   10512 / 11181 (the resident call's own repeat gap: 2 / 12 / 1 us at S = 1).
// Those runs take one trial per iteration, so every slot past the first is six launches that return at once; a rejected
// trial costs S = 1 one more look (a stream wait) instead.  1 is the best of the three, or level with 2, at every size.
enum { kTrialSlots = 1 };
thread_local int t_trial_slots = 0;  // vsg_debug_local_ba_trial_slots: 0 = kTrialSlots

#include "vsg_ba_kernels.inc"

struct FinalArgs {
  const int32_t *slots;
  float *pos;  // the store's, written
  const vsg_pose_se3 *Tcw;
  const int32_t *opt_of;
  uint8_t *erase;
  double *chi2;
  vsg_pose_se3d *kf_out;
  float *pos_out;
};

// The reduced system in ONE workgroup: a right-looking LDL^T sweep over the lower triangle in global memory (6 x 128
// keyframes are 768 rows, 4.7 MB of doubles: past LDS, inside L2), column k's multipliers staged in LDS, then the forward
// and backward substitutions with the right-hand side in LDS.  Element (i, j) takes -(L_ik L_jk) D_k in ascending k, which
// is what lba::solve_reduced_host's left-looking loops give it.  One code path for every n <= 6 kMaxOptKf.
__global__ __launch_bounds__(lba::kSolveThreads) void k_solve(lba::Prob p, int it, int q) {
  enum { kN = 6 * lba::kMaxOptKf, T = lba::kSolveThreads, W = lba::kSolveTile };
  __shared__ double l[kN], D[kN], y[kN];
  __shared__ int bad;
  if (!lba::run_trial(*p.S, it, q)) return;
  const int n = p.n, tid = threadIdx.x, tx = tid % W, ty = tid / W;
  double *M = p.M;
  if (tid == 0) bad = 0;
  for (int k = 0; k < n; k++) {
    __syncthreads();  // step k - 1's updates are visible; its readers are done with l
    const double d = M[(size_t)k * n + k];
    if (tid == 0) {
      D[k] = d;
      if (d <= 0.0) bad = 1;
    }
    for (int i = k + 1 + tid; i < n; i += T) {
      const double v = M[(size_t)i * n + k] / d;
      M[(size_t)i * n + k] = v, l[i] = v;
    }
    __syncthreads();
    for (int i = k + 1 + ty; i < n; i += T / W) {
      const double li = l[i];
      for (int j = k + 1 + tx; j <= i; j += W) M[(size_t)i * n + j] = M[(size_t)i * n + j] - (li * l[j]) * d;
    }
  }
  for (int i = tid; i < n; i += T) y[i] = p.bs[i];
  for (int k = 0; k < n; k++) {
    __syncthreads();
    const double yk = y[k];
    for (int i = k + 1 + tid; i < n; i += T) y[i] = y[i] - M[(size_t)i * n + k] * yk;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) y[i] = y[i] / D[i];
  for (int k = n - 1; k >= 0; k--) {
    __syncthreads();
    const double xk = y[k];
    for (int i = tid; i < k; i += T) y[i] = y[i] - M[(size_t)k * n + i] * xk;
  }
  __syncthreads();
  for (int i = tid; i < n; i += T) p.xp[i] = y[i];
  if (tid == 0) *p.ok2 = bad ? 0 : 1;
}

// workgroups [0, Gp): one lane per point; workgroup Gp: the optimised keyframes' oplus
__global__ __launch_bounds__(lba::kThreads) void k_backsub(lba::Prob p, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, tid = threadIdx.x, cur = p.S->cur;
  if (g == p.Gp) {
    if (tid < p.Ko) lba::oplus_kf(p, tid, cur);
    return;
  }
  const int pt = g * lba::kThreads + tid;
  double v = pt < p.P ? lba::backsub_point(p, pt, cur, p.S->lambda) : 0.0;
  block_tree<1, false>(&v, lds);
  if (tid == 0) p.scalePart[g] = v;
}

// the classification (:2296-2340) and the recovery (:2398-2414)
__global__ __launch_bounds__(lba::kThreads) void k_final(lba::Prob p, FinalArgs A) {
  const int i = blockIdx.x * lba::kThreads + threadIdx.x, cur = p.S->cur;
  if (i < p.E) lba::classify_edge(p, i, cur, A.erase, A.chi2);
  if (i < p.K) A.kf_out[i] = A.opt_of[i] >= 0 ? lba::pose_out(p.est[cur][i]) : lba::pose_widened(A.Tcw[i]);
  if (i < p.P) {
    const size_t s = (size_t)A.slots[i];
    const bool vertex = p.p_off[i] != p.p_off[i + 1];
    for (int d = 0; d < 3; d++) {
      const float v = vertex ? pose::canonf((float)p.X[cur][3 * (size_t)i + d]) : A.pos[3 * s + d];
      A.pos_out[3 * (size_t)i + d] = v;
      if (vertex) A.pos[3 * s + d] = v;
    }
  }
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
  if (!store_fields(mp, &F) || n_kf < 0 || !inv_level_sigma2 || !kf_Tcw_out || !erase || !res) return VSG_ERR_INVALID;
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
  int rc = lba::check_and_build(
      n_points, slots, obs_off, obs_kf, obs_idx, n_kf, kf_n.data(), nleft.data(),
      [&](int k, int i) { return (int)kfs[k]->h_kps[(size_t)i].octave; }, kf_fixed, F.capacity, nlevels, iterations,
      stop_flag, &T, &ran);
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
  const SetupArgs &SA = G.SA;
  uint8_t *hp = G.hp, *dp = G.dp, *dv = G.dv;
  const size_t in_bytes = G.in_bytes, Ge = G.Ge, Gp = G.Gp, oErase = G.out_off[0], oChi2 = G.out_off[1], oKfOut = G.out_off[2],
               oPosOut = G.out_off[3];
  lba::State *mirror = G.mirror, *mirror_dev = G.mirror_dev;
  FinalArgs FA;
  FA.slots = SA.slots, FA.pos = F.pos, FA.Tcw = G.Tcw_dev, FA.opt_of = G.opt_of_dev;
  FA.erase = dp + oErase, FA.chi2 = (double *)(dp + oChi2), FA.kf_out = (vsg_pose_se3d *)(dp + oKfOut), FA.pos_out = (float *)(dp + oPosOut);

  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, c->stream));
  // from here on an error waits for the stream before it returns: the arenas belong to the next call
  hipStream_t st = c->stream;
  const dim3 B(lba::kThreads);
  const unsigned gAll = G.gAll;
  const int Gs = G.Gs;
  const int S = t_trial_slots > 0 ? t_trial_slots : (int)kTrialSlots;
  hipLaunchKernelGGL(k_setup, dim3(gAll), B, 0, st, p, SA);
  bool failed = false, stopped = false;
  for (int it = 0; it < iterations && !failed; it++) {
    hipLaunchKernelGGL(k_linearise<lba::HuberLocal>, dim3((unsigned)Ge), B, 0, st, p, it, lba::HuberLocal());
    hipLaunchKernelGGL(k_gather, dim3((unsigned)(Gp + Ko)), B, 0, st, p, it);
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, p, it, mirror_dev);
    bool closed = false;
    for (int q = 0; q < lba::kTrials && !closed && !failed;) {
      for (int s = 0; s < S && q < lba::kTrials; s++, q++) {
        hipLaunchKernelGGL(k_trial_edges, dim3((unsigned)Ge), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_schur, dim3((unsigned)(Gs + (int)Ko)), B, 0, st, p, it, q, Gs);
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(lba::kSolveThreads), 0, st, p, it, q);
        hipLaunchKernelGGL(k_backsub, dim3((unsigned)(Gp + 1)), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_error<lba::HuberLocal>, dim3((unsigned)Ge), B, 0, st, p, it, q, lba::HuberLocal());
        hipLaunchKernelGGL(k_decide, dim3(1), dim3(1), 0, st, p, it, q, mirror_dev);
      }
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
