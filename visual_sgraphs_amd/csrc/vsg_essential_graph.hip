// vsg_essential_graph.hip -- Optimizer::OptimizeEssentialGraph, first overload (Optimizer.cc:2456-2734), on resident map
// points: vsg_mappoints_optimize_essential_graph, and the point correction it shares with LoopClosing::CorrectLoop
// (LoopClosing.cc:1060-1064): vsg_mappoints_correct_sim3 (include/vsg_orb.h).  The arithmetic is csrc/vsg_essential_graph.h,
// shared with the host build bit for bit; this file adds the kernels around its per-item functions and the enqueue policy.
//
// KERNEL BOUNDARIES ON THE CALLING THREAD'S STREAM ARE THE ONLY SYNCHRONISATION BETWEEN WORKGROUPS, as in vsg_local_ba.hip
// and vsg_global_ba.hip: no grid-wide barrier, no cooperative launch, no flag between workgroups, nothing spins.  The
// Levenberg controller (lba::State) lives in device memory, is written by the one-lane steps k_eg_begin and k_eg_decide
// alone, and is read first by every kernel, the solver's included, which returns at once when its iteration or trial is not
// to run.  The host's enqueue policy is csrc/vsg_lm_driver.h, the bundle adjustments' too.
//
// Per iteration: k_eg_linearise (ONE WAVE PER EDGE: lanes 0-27 each take one (vertex, column, sign) of the numeric Jacobian,
// lane 28 the error itself -- 29 evaluations of Sim3::log() side by side -- then the 64 lanes split the 119 entries of the
// edge's blocks; errors and Jacobians go through LDS), k_eg_gather (the chi2 tree and b), k_eg_begin.  Per trial:
// k_eg_assemble (the dense lower triangle of H + lambda I from the per-edge blocks, one lane per entry, empty blocks as
// zeros), THE SOLVE (vsg_ldl_chain.inc, the global BA's chain, one copy of its text), k_eg_oplus, k_eg_error, k_eg_decide.
// Then k_eg_final: the estimates, chi2 per edge, and the correction of the listed points in the store.
// All stores are plain vector stores; there is no atomic of any kind.
#include <cstring>

#include "vsg_block_tree.h"
#include "vsg_essential_graph.h"
#include "vsg_frame_int.h"
#include "vsg_lm_driver.h"

using namespace vsg;

namespace {

enum { kThreads = lba::kThreads, W = gba::kPanel, TS = gba::kTile, WP = W + 1, kEdgesPerGroup = kThreads / pose::kWave };
#include "vsg_ldl_chain.inc"

struct FinalArgs {
  const int32_t *opt_of, *slots, *point_ref;
  float *pos;  // the store's
  vsg_sim3d *kf_out;
  double *chi2;  // nullptr: not asked for
  float *pos_out;
  int P;
};

struct CorrectArgs {
  const int32_t *slots, *point_ref;
  const vsg_sim3d *from, *to_inv;
  float *pos, *pos_out;
  int P;
};

// the measurements (one lane per edge), both estimate buffers (one lane per keyframe), the 14 factors of the Jacobian
__global__ __launch_bounds__(kThreads) void k_eg_setup(eg::Prob p) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i < p.E) p.meas[i] = eg::measurement(p.Scw, p.nonc, p.has_nonc, p.e_i[i], p.e_j[i], p.e_loop[i] != 0);
  if (i < p.K) p.est[0][i] = p.est[1][i] = sim3opt::sim3_of(p.Scw[i]);
  if (i < eg::kPert) p.pert[i] = eg::perturbation(i, p.fix_scale != 0);
}

// one wave per edge, kEdgesPerGroup edges per workgroup
__global__ __launch_bounds__(kThreads) void k_eg_linearise(eg::Prob p, int it) {
  __shared__ double err[kEdgesPerGroup][eg::kSlots][eg::kDim], J[kEdgesPerGroup][2][eg::kDim][eg::kDim];
  if (!lba::run_iteration(*p.S, it)) return;
  const int lane = threadIdx.x & (pose::kWave - 1), wave = threadIdx.x / pose::kWave, e = blockIdx.x * kEdgesPerGroup + wave;
  const bool live = e < p.E;
  if (live && lane < eg::kSlots) {
    double r[eg::kDim];
    eg::slot_error(p, e, lane, p.S->cur, r);
#pragma unroll
    for (int k = 0; k < eg::kDim; k++) err[wave][lane][k] = r[k];
  }
  __syncthreads();
  if (live) {
    for (int x = lane; x < 2 * eg::kDim * eg::kDim; x += pose::kWave) {
      const int v = x / (eg::kDim * eg::kDim), r = (x / eg::kDim) % eg::kDim, d = x % eg::kDim;
      J[wave][v][r][d] = eg::jacobian_entry(err[wave][v * eg::kPert + 2 * d][r], err[wave][v * eg::kPert + 2 * d + 1][r]);
    }
    if (lane == 0) p.chi2[e] = eg::edge_chi2(err[wave][2 * eg::kPert]);
  }
  __syncthreads();
  if (live) {
    const int oi = p.e_oi[e], oj = p.e_oj[e];
    for (int x = lane; x < eg::kBlock; x += pose::kWave)
      if (eg::block_entry_live(oi, oj, x))
        p.blocks[(size_t)e * eg::kBlock + x] = eg::block_entry(&J[wave][0][0][0], &J[wave][1][0][0], eg::kDim, err[wave][2 * eg::kPert], x);
  }
}

// workgroups [0, Ge): the chi2 of kThreads edges through the tree; [Ge, ...): one lane per row of b
__global__ __launch_bounds__(kThreads) void k_eg_gather(eg::Prob p, int it) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_iteration(*p.S, it)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < p.Ge) {
    const int e = g * kThreads + tid;
    double v = e < p.E ? p.chi2[e] : 0.0;
    block_tree<1, false>(&v, lds);
    if (tid == 0) p.chiPart[g] = v;
    return;
  }
  const int r = (g - p.Ge) * kThreads + tid;
  if (r < p.n) p.b[r] = eg::gather_b(p, r);
}

__global__ void k_eg_begin(eg::Prob p, int it, lba::State *mirror) {
  if (!lba::run_iteration(*p.S, it)) return;
  eg::begin_iteration(p, it);
  *mirror = *p.S;
}

// one lane per entry of a 7 x 7 block of the lower triangle
__global__ __launch_bounds__(kThreads) void k_eg_assemble(eg::Prob p, int it, int q) {
  if (!lba::run_trial(*p.S, it, q)) return;
  const long long x = (long long)blockIdx.x * kThreads + threadIdx.x;
  const int blk = (int)(x / (eg::kDim * eg::kDim)), ent = (int)(x % (eg::kDim * eg::kDim));
  if (blk < p.nb) eg::assemble_entry(p, blk, ent / eg::kDim, ent % eg::kDim, p.S->lambda);
}

__global__ __launch_bounds__(kThreads) void k_eg_oplus(eg::Prob p, int it, int q) {
  if (!lba::run_trial(*p.S, it, q)) return;
  const int a = blockIdx.x * kThreads + threadIdx.x;
  if (a < p.Ko) eg::oplus_vertex(p, a, p.S->cur);
}

__global__ __launch_bounds__(kThreads) void k_eg_error(eg::Prob p, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  double v = e < p.E ? eg::edge_cost(p, e, p.S->cur ^ 1) : 0.0;
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.chiPart[blockIdx.x] = v;
}

__global__ void k_eg_decide(eg::Prob p, int it, int q, lba::State *mirror) {
  if (!lba::run_trial(*p.S, it, q)) return;
  eg::decide(p);
  *mirror = *p.S;
}

// the write-back (:2690-2731): the estimates, chi2 per edge at them, the listed points through their reference keyframe
__global__ __launch_bounds__(kThreads) void k_eg_final(eg::Prob p, FinalArgs A) {
  const int i = blockIdx.x * kThreads + threadIdx.x, cur = p.S->cur;
  if (i < p.K) A.kf_out[i] = A.opt_of[i] >= 0 ? sim3opt::sim3d_canon(p.est[cur][i]) : p.Scw[i];
  if (A.chi2 && i < p.E) A.chi2[i] = pose::canon(eg::edge_cost(p, i, cur));
  if (i < A.P) {
    const size_t s = (size_t)A.slots[i];
    const int r = A.point_ref[i];
    const float in[3] = {A.pos[3 * s], A.pos[3 * s + 1], A.pos[3 * s + 2]};
    float out[3];
    eg::correct_point(sim3opt::sim3_of(p.Scw[r]), sim3opt::sim3_inverse(p.est[cur][r]), in, out);
    for (int d = 0; d < 3; d++) A.pos[3 * s + d] = out[d], A.pos_out[3 * (size_t)i + d] = out[d];
  }
}

__global__ __launch_bounds__(kThreads) void k_eg_correct(CorrectArgs A) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= A.P) return;
  const size_t s = (size_t)A.slots[i];
  const int r = A.point_ref[i];
  const float in[3] = {A.pos[3 * s], A.pos[3 * s + 1], A.pos[3 * s + 2]};
  float out[3];
  eg::correct_point(sim3opt::sim3_of(A.from[r]), sim3opt::sim3_of(A.to_inv[r]), in, out);
  for (int d = 0; d < 3; d++) A.pos[3 * s + d] = out[d], A.pos_out[3 * (size_t)i + d] = out[d];
}

}  // namespace

extern "C" {

int vsg_mappoints_optimize_essential_graph(vsg_mappoints *mp, int n_kf, const vsg_sim3d *kf_Scw, const vsg_sim3d *kf_non_corrected,
                                           const uint8_t *kf_has_non_corrected, const uint8_t *kf_fixed, int n_edges,
                                           const int32_t *edge_i, const int32_t *edge_j, const uint8_t *edge_loop, int fix_scale,
                                           int iterations, int n_points, const int32_t *slots, const int32_t *point_ref,
                                           vsg_sim3d *kf_Scw_out, float *world_pos_out, double *chi2,
                                           vsg_essential_graph_result *res) {
  StoreFields F;
  memset(&F, 0, sizeof(F));
  if (mp && !store_fields(mp, &F)) return VSG_ERR_INVALID;
  eg::Topology T;
  int ran = 0;
  int rc = eg::check_and_build(n_kf, kf_Scw, kf_non_corrected, kf_has_non_corrected, kf_fixed, n_edges, edge_i, edge_j, edge_loop,
                               fix_scale, iterations, n_points, slots, point_ref, mp ? F.capacity : -1, kf_Scw_out, res, &T, &ran);
  if (rc != VSG_OK) return rc;
  if (!ran) {
    for (int k = 0; k < n_kf; k++) kf_Scw_out[k] = kf_Scw[k];
    eg::fill_result(res, T, nullptr);
    return VSG_OK;
  }
  // everything the kernels index has been bounded; nothing has been enqueued
  int device = F.device;
  if (!mp && hipGetDevice(&device) != hipSuccess) return VSG_ERR_NO_DEVICE;
  ThreadCtx *c = thread_ctx(device, &rc);
  if (!c) return rc;
  const size_t E = (size_t)T.E, K = (size_t)T.K, Ko = (size_t)T.Ko, P = (size_t)n_points, n = eg::kDim * Ko, nb = T.blk_a.size(),
               Ge = (E + kThreads - 1) / kThreads, Gb = (n + kThreads - 1) / kThreads;
  Stage in;
  const size_t oEi = in.add(E * 4), oEj = in.add(E * 4), oEoi = in.add(E * 4), oEoj = in.add(E * 4), oEloop = in.add(E),
               oBa = in.add(nb * 4), oBb = in.add(nb * 4), oBoff = in.add((nb + 1) * 4), oBent = in.add(T.blk_ent.size() * 4),
               oVoff = in.add((Ko + 1) * 4), oVent = in.add(T.v_ent.size() * 4), oOptKf = in.add(Ko * 4), oOptOf = in.add(K * 4),
               oScw = in.add(K * sizeof(vsg_sim3d)), oNonc = in.add(K * sizeof(vsg_sim3d)), oHas = in.add(K), oSlots = in.add(P * 4),
               oRef = in.add(P * 4), oState = in.add(sizeof(lba::State)), oOk2 = in.add(4);
  const size_t in_bytes = in.total;
  Stage out = in;
  const size_t oMirror = out.add(sizeof(lba::State)), oKfOut = out.add(K * sizeof(vsg_sim3d)), oChi2 = out.add(E * 8),
               oPosOut = out.add(P * 12);
  Stage dev = in;
  const size_t dEst0 = dev.add(K * sizeof(eg::Sim3)), dEst1 = dev.add(K * sizeof(eg::Sim3)), dMeas = dev.add(E * sizeof(eg::Sim3)),
               dPert = dev.add(eg::kPert * sizeof(eg::Sim3)), dBlocks = dev.add(E * eg::kBlock * 8), dChi = dev.add(E * 8),
               dM = dev.add(n * n * 8), dB = dev.add(n * 8), dXp = dev.add(n * 8), dD = dev.add(n * 8), dY = dev.add(n * 8),
               dAcc = dev.add(n * 8), dChiPart = dev.add(Ge * 8);
  rc = ctx_reserve(c, out.total, dev.total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin, *dv = c->d_buf;
  put(hp, oEi, T.e_i), put(hp, oEj, T.e_j), put(hp, oEoi, T.e_oi), put(hp, oEoj, T.e_oj), put(hp, oEloop, T.e_loop);
  put(hp, oBa, T.blk_a), put(hp, oBb, T.blk_b), put(hp, oBoff, T.blk_off), put(hp, oBent, T.blk_ent), put(hp, oVoff, T.v_off);
  put(hp, oVent, T.v_ent), put(hp, oOptKf, T.opt_kf), put(hp, oOptOf, T.opt_of);
  memcpy(hp + oScw, kf_Scw, K * sizeof(vsg_sim3d));
  memcpy(hp + oHas, kf_has_non_corrected, K);
  memset(hp + oNonc, 0, K * sizeof(vsg_sim3d));
  for (size_t k = 0; k < K; k++)
    if (kf_has_non_corrected[k]) ((vsg_sim3d *)(hp + oNonc))[k] = kf_non_corrected[k];
  if (P) memcpy(hp + oSlots, slots, P * 4), memcpy(hp + oRef, point_ref, P * 4);
  memset(hp + oState, 0, sizeof(lba::State));
  *(int32_t *)(hp + oOk2) = 1;
  lba::State *mirror = (lba::State *)(hp + oMirror), *mirror_dev = (lba::State *)(dp + oMirror);
  memset(mirror, 0, sizeof(*mirror));

  eg::Prob p;
  memset(&p, 0, sizeof(p));
  p.K = T.K, p.Ko = T.Ko, p.E = T.E, p.n = (int)n, p.nb = (int)nb, p.Ge = (int)Ge, p.iterations = iterations, p.fix_scale = fix_scale;
  p.e_i = (const int32_t *)(dv + oEi), p.e_j = (const int32_t *)(dv + oEj), p.e_oi = (const int32_t *)(dv + oEoi);
  p.e_oj = (const int32_t *)(dv + oEoj), p.e_loop = dv + oEloop, p.blk_a = (const int32_t *)(dv + oBa), p.blk_b = (const int32_t *)(dv + oBb);
  p.blk_off = (const int32_t *)(dv + oBoff), p.blk_ent = (const int32_t *)(dv + oBent), p.v_off = (const int32_t *)(dv + oVoff);
  p.v_ent = (const int32_t *)(dv + oVent), p.opt_kf = (const int32_t *)(dv + oOptKf), p.Scw = (const vsg_sim3d *)(dv + oScw);
  p.nonc = (const vsg_sim3d *)(dv + oNonc), p.has_nonc = dv + oHas, p.meas = (eg::Sim3 *)(dv + dMeas);
  p.est[0] = (eg::Sim3 *)(dv + dEst0), p.est[1] = (eg::Sim3 *)(dv + dEst1), p.pert = (eg::Sim3 *)(dv + dPert);
  p.blocks = (double *)(dv + dBlocks), p.chi2 = (double *)(dv + dChi), p.M = (double *)(dv + dM), p.b = (double *)(dv + dB);
  p.xp = (double *)(dv + dXp), p.chiPart = (double *)(dv + dChiPart), p.ok2 = (int32_t *)(dv + oOk2), p.S = (lba::State *)(dv + oState);
  Solve sv;
  sv.n = (int)n, sv.M = p.M, sv.bs = p.b, sv.xp = p.xp, sv.D = (double *)(dv + dD), sv.y = (double *)(dv + dY);
  sv.acc = (double *)(dv + dAcc), sv.ok2 = p.ok2, sv.S = p.S;
  FinalArgs FA;
  FA.opt_of = (const int32_t *)(dv + oOptOf), FA.slots = (const int32_t *)(dv + oSlots), FA.point_ref = (const int32_t *)(dv + oRef);
  FA.pos = F.pos, FA.kf_out = (vsg_sim3d *)(dp + oKfOut), FA.chi2 = chi2 ? (double *)(dp + oChi2) : nullptr;
  FA.pos_out = (float *)(dp + oPosOut), FA.P = n_points;

  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, c->stream));
  hipStream_t st = c->stream;
  const dim3 B(kThreads);
  const size_t most = E > K ? (E > P ? E : P) : (K > P ? K : P), most14 = most > (size_t)eg::kPert ? most : (size_t)eg::kPert;
  const unsigned gAll = (unsigned)((most14 + kThreads - 1) / kThreads), gLin = (unsigned)((E + kEdgesPerGroup - 1) / kEdgesPerGroup);
  const unsigned gAsm = (unsigned)((nb * eg::kDim * eg::kDim + kThreads - 1) / kThreads), gKo = (unsigned)((Ko + kThreads - 1) / kThreads);
  hipLaunchKernelGGL(k_eg_setup, dim3(gAll), B, 0, st, p);
  lba::State Sfin;
  const bool done = lm::run(
      st, mirror, iterations, lm::kTrialSlots, nullptr,
      [&](int it) {
        hipLaunchKernelGGL(k_eg_linearise, dim3(gLin), B, 0, st, p, it);
        hipLaunchKernelGGL(k_eg_gather, dim3((unsigned)(Ge + Gb)), B, 0, st, p, it);
        hipLaunchKernelGGL(k_eg_begin, dim3(1), dim3(1), 0, st, p, it, mirror_dev);
      },
      [&](int it, int q) {
        hipLaunchKernelGGL(k_eg_assemble, dim3(gAsm), B, 0, st, p, it, q);
        enqueue_solve(st, sv, it, q);
        hipLaunchKernelGGL(k_eg_oplus, dim3(gKo), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_eg_error, dim3((unsigned)Ge), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_eg_decide, dim3(1), dim3(1), 0, st, p, it, q, mirror_dev);
      },
      [&] { hipLaunchKernelGGL(k_eg_final, dim3(gAll), B, 0, st, p, FA); },
      &Sfin);
  if (!done) return VSG_ERR_HIP;
  eg::fill_result(res, T, &Sfin);
  memcpy(kf_Scw_out, hp + oKfOut, K * sizeof(vsg_sim3d));
  if (chi2) memcpy(chi2, hp + oChi2, E * 8);
  if (world_pos_out && P) memcpy(world_pos_out, hp + oPosOut, P * 12);
  return VSG_OK;
}

int vsg_mappoints_correct_sim3(vsg_mappoints *mp, int n_points, const int32_t *slots, const int32_t *point_ref, int n_ref,
                               const vsg_sim3d *S_from, const vsg_sim3d *S_to_inverse, float *world_pos_out) {
  StoreFields F;
  if (!store_fields(mp, &F) || n_points < 0 || n_ref < 0) return VSG_ERR_INVALID;
  if (n_points == 0) return VSG_OK;
  if (!S_from || !S_to_inverse || !eg::check_points(n_points, slots, point_ref, F.capacity, n_ref)) return VSG_ERR_INVALID;
  for (int r = 0; r < n_ref; r++)
    if (!eg::sim3_ok(S_from[r]) || !eg::sim3_ok(S_to_inverse[r])) return VSG_ERR_INVALID;
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(F.device, &rc);
  if (!c) return rc;
  const size_t P = (size_t)n_points, R = (size_t)n_ref;
  Stage st;
  const size_t oSlots = st.add(P * 4), oRef = st.add(P * 4), oFrom = st.add(R * sizeof(vsg_sim3d)), oTo = st.add(R * sizeof(vsg_sim3d)),
               oOut = st.add(P * 12);
  rc = ctx_reserve(c, st.total, 0);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin;
  memcpy(hp + oSlots, slots, P * 4), memcpy(hp + oRef, point_ref, P * 4);
  memcpy(hp + oFrom, S_from, R * sizeof(vsg_sim3d)), memcpy(hp + oTo, S_to_inverse, R * sizeof(vsg_sim3d));
  CorrectArgs A;
  A.slots = (const int32_t *)(dp + oSlots), A.point_ref = (const int32_t *)(dp + oRef), A.from = (const vsg_sim3d *)(dp + oFrom);
  A.to_inv = (const vsg_sim3d *)(dp + oTo), A.pos = F.pos, A.pos_out = (float *)(dp + oOut), A.P = n_points;
  hipLaunchKernelGGL(k_eg_correct, dim3((unsigned)((P + kThreads - 1) / kThreads)), dim3(kThreads), 0, c->stream, A);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  if (world_pos_out) memcpy(world_pos_out, hp + oOut, P * 12);
  return VSG_OK;
}

}  // extern "C"
