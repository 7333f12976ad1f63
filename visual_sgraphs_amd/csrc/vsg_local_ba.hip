// vsg_local_ba.hip -- the visual part of Optimizer::LocalBundleAdjustment (Optimizer.cc:1454-2454) on resident keyframes
// and resident map points: vsg_mappoints_local_bundle_adjustment (include/vsg_orb.h).  The arithmetic is csrc/vsg_local_ba.h,
// shared with the host build bit for bit; this file adds the kernels around its per-item functions, the reduction tree on
// the wavefronts, the reduced solve's sweep and the enqueue policy.
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

struct KfTab {
  const KeyPointPOD *kps;
  const float *ur;  // nullptr: every mvuRight is -1
};

struct SetupArgs {
  const KfTab *tab;
  const int32_t *e_idx, *slots;
  const float *pos;  // the store's GetWorldPos()
  float sig[16];
};

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

// the fixed tree of vsg_pose_opt.h over one workgroup of lba::kThreads lanes: butterfly over the wave, the waves serially
template <int N, bool kMax>
__device__ __forceinline__ void block_tree(double *acc, double *lds) {
  const int lane = threadIdx.x & (pose::kWave - 1), wave = threadIdx.x / pose::kWave;
#pragma unroll
  for (int k = 0; k < N; k++) {
    double v = acc[k];
#pragma unroll
    for (int s = 1; s < pose::kWave; s <<= 1) {
      const double o = __shfl_xor(v, s, pose::kWave);
      v = kMax ? (v < o ? o : v) : v + o;
    }
    acc[k] = v;
  }
  __syncthreads();  // the previous tree's readers are done with lds
  if (lane == 0) {
#pragma unroll
    for (int k = 0; k < N; k++) lds[wave * N + k] = acc[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) {
    double t = lds[k];
#pragma unroll
    for (int w = 1; w < pose::kWaves; w++) {
      const double o = lds[w * N + k];
      t = kMax ? (t < o ? o : t) : t + o;
    }
    acc[k] = t;
  }
}

// :1850-1948 for the listed observations: the measurement, the information and the kind of every edge; the points'
// estimates from the store into both buffers
__global__ __launch_bounds__(lba::kThreads) void k_setup(lba::Prob p, SetupArgs A) {
  const int i = blockIdx.x * lba::kThreads + threadIdx.x;
  bool mono = false, stereo = false;
  if (i < p.E) {
    const KfTab t = A.tab[p.e_kf[i]];
    const int idx = A.e_idx[i];
    const KeyPointPOD kp = t.kps[idx];
    const float ur = t.ur ? t.ur[idx] : -1.0f;
    stereo = ur >= 0, mono = !stereo;
    const size_t E = (size_t)p.E;
    p.obs[i] = (double)kp.x, p.obs[E + i] = (double)kp.y, p.obs[2 * E + i] = stereo ? (double)ur : 0.0;
    const int o = kp.octave & 15;
    p.w[i] = (double)A.sig[o];
    p.flag[i] = stereo ? lba::kStereo : 0;
    p.chi2[i] = 0.0;
  }
  // the two edge counts: one integer atomic per wavefront and kind
  const unsigned long long ms = __ballot(stereo), mm = __ballot(mono);
  if ((threadIdx.x & (pose::kWave - 1)) == 0) {
    if (ms) atomicAdd(&p.S->n_stereo, __popcll(ms));
    if (mm) atomicAdd(&p.S->n_mono, __popcll(mm));
  }
  if (i < p.P) {
    const size_t s = (size_t)A.slots[i];
    for (int d = 0; d < 3; d++) p.X[0][3 * (size_t)i + d] = p.X[1][3 * (size_t)i + d] = (double)A.pos[3 * s + d];
  }
  if (i < p.K) p.est[1][i] = p.est[0][i];
}

__global__ __launch_bounds__(lba::kThreads) void k_linearise(lba::Prob p, int it) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_iteration(*p.S, it)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  double v = e < p.E ? lba::linearise_edge(p, e, p.S->cur) : 0.0;
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.chiPart[blockIdx.x] = v;
}

// workgroups [0, Gp): one lane per point; [Gp, Gp + Ko): one workgroup per optimised keyframe
__global__ __launch_bounds__(lba::kThreads) void k_gather(lba::Prob p, int it) {
  __shared__ double lds[pose::kWaves * lba::kHppC];
  if (!lba::run_iteration(*p.S, it)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < p.Gp) {
    const int pt = g * lba::kThreads + tid;
    double m = pt < p.P ? lba::gather_point(p, pt) : 0.0;
    block_tree<1, true>(&m, lds);
    if (tid == 0) p.maxPart[g] = m;
    return;
  }
  double acc[lba::kHppC];
  lba::gather_kf_partial(p, g - p.Gp, tid, acc);
  block_tree<lba::kHppC, false>(acc, lds);
  if (tid == 0) lba::gather_kf_store(p, g - p.Gp, acc);
}

__global__ void k_begin(lba::Prob p, int it, lba::State *mirror) {
  if (!lba::run_iteration(*p.S, it)) return;
  lba::begin_iteration(p, it);
  *mirror = *p.S;
}

__global__ __launch_bounds__(lba::kThreads) void k_trial_edges(lba::Prob p, int it, int q) {
  if (!lba::run_trial(*p.S, it, q)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  if (e < p.E) lba::trial_edge(p, e, p.S->lambda);
}

enum { kBlocksPerGroup = lba::kThreads / 36 };  // Schur blocks per workgroup, one lane per entry

// workgroups [0, Gs): kBlocksPerGroup Schur blocks each; [Gs, Gs + Ko): bschur of one optimised keyframe
__global__ __launch_bounds__(lba::kThreads) void k_schur(lba::Prob p, int it, int q, int Gs) {
  __shared__ double lds[pose::kWaves * lba::kC];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int g = blockIdx.x, tid = threadIdx.x;
  if (g < Gs) {
    const int blk = g * kBlocksPerGroup + tid / 36, ent = tid % 36;
    if (tid < kBlocksPerGroup * 36 && blk < p.nb) lba::schur_entry(p, blk, ent / 6, ent % 6, p.S->lambda);
    return;
  }
  double acc[lba::kC];
  lba::bschur_partial(p, g - Gs, tid, acc);
  block_tree<lba::kC, false>(acc, lds);
  if (tid == 0) lba::bschur_store(p, g - Gs, acc);
}

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

__global__ __launch_bounds__(lba::kThreads) void k_error(lba::Prob p, int it, int q) {
  __shared__ double lds[pose::kWaves];
  if (!lba::run_trial(*p.S, it, q)) return;
  const int e = blockIdx.x * lba::kThreads + threadIdx.x;
  double v = 0.0;
  if (e < p.E) {
    double err[3], Xc[3], rho1;
    v = lba::edge_cost(p, e, p.S->cur ^ 1, err, Xc, &rho1);
  }
  block_tree<1, false>(&v, lds);
  if (threadIdx.x == 0) p.chiPart[blockIdx.x] = v;
}

__global__ void k_decide(lba::Prob p, int it, int q, lba::State *mirror) {
  if (!lba::run_trial(*p.S, it, q)) return;
  lba::decide(p);
  *mirror = *p.S;
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

template <class T>
void put(uint8_t *base, size_t off, const std::vector<T> &v) {
  if (!v.empty()) memcpy(base + off, v.data(), v.size() * sizeof(T));
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
  const size_t E = (size_t)T.E, P = (size_t)T.P, K = (size_t)T.K, Ko = (size_t)T.Ko, n = 6 * Ko, nb = T.b_i.size(),
               NP = T.pair_a.size(), Ge = (E + lba::kThreads - 1) / lba::kThreads, Gp = (P + lba::kThreads - 1) / lba::kThreads;
  // the pinned arena: the lists and start values (copied to the device arena once), then what the kernels write back
  Stage in;
  const size_t oEkf = in.add(E * 4), oEpt = in.add(E * 4), oEopt = in.add(E * 4), oEidx = in.add(E * 4), oPoff = in.add((P + 1) * 4),
               oSlots = in.add(P * 4), oKoff = in.add((Ko + 1) * 4), oKedge = in.add(T.k_edge.size() * 4), oBi = in.add(nb * 4),
               oBj = in.add(nb * 4), oBoff = in.add((nb + 1) * 4), oPa = in.add(NP * 4), oPb = in.add(NP * 4), oOptKf = in.add(Ko * 4),
               oOptOf = in.add(K * 4), oCam = in.add(K * sizeof(lba::Cam)), oEst0 = in.add(K * sizeof(lba::Est)),
               oTab = in.add(K * sizeof(KfTab)), oTcw = in.add(K * sizeof(vsg_pose_se3)), oState = in.add(sizeof(lba::State)),
               oOk2 = in.add(4);
  const size_t in_bytes = in.total;
  Stage out = in;
  const size_t oMirror = out.add(sizeof(lba::State)), oErase = out.add(E), oChi2 = out.add(E * 8),
               oKfOut = out.add(K * sizeof(vsg_pose_se3d)), oPosOut = out.add(P * 12);
  Stage dev = in;  // the device arena: the copy of the inputs, then the scratch
  const size_t dEst1 = dev.add(K * sizeof(lba::Est)), dX0 = dev.add(P * 24), dX1 = dev.add(P * 24), dObs = dev.add(E * 24),
               dW = dev.add(E * 8), dFlag = dev.add(E), dChi = dev.add(E * 8), dHpl = dev.add(E * 8 * lba::kHpl),
               dHppC = dev.add(E * 8 * lba::kHppC), dHllC = dev.add(E * 8 * lba::kHllC), dBD = dev.add(E * 8 * lba::kHpl),
               dC = dev.add(E * 8 * lba::kC), dHpp = dev.add(Ko * 8 * lba::kHppC), dHll = dev.add(P * 8 * lba::kHllC),
               dM = dev.add(n * n * 8), dBs = dev.add(n * 8), dXp = dev.add(n * 8), dChiPart = dev.add(Ge * 8),
               dMaxPart = dev.add(Gp * 8), dMaxKf = dev.add(Ko * 8), dScale = dev.add(Gp * 8);
  rc = ctx_reserve(c, out.total, dev.total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin, *dv = c->d_buf;
  put(hp, oEkf, T.e_kf), put(hp, oEpt, T.e_pt), put(hp, oEopt, T.e_opt), put(hp, oEidx, T.e_idx), put(hp, oPoff, T.p_off);
  memcpy(hp + oSlots, slots, P * 4);
  put(hp, oKoff, T.k_off), put(hp, oKedge, T.k_edge), put(hp, oBi, T.b_i), put(hp, oBj, T.b_j), put(hp, oBoff, T.b_off);
  put(hp, oPa, T.pair_a), put(hp, oPb, T.pair_b), put(hp, oOptKf, T.opt_kf), put(hp, oOptOf, T.opt_of);
  lba::Cam *cam = (lba::Cam *)(hp + oCam);
  lba::Est *est0 = (lba::Est *)(hp + oEst0);
  KfTab *tab = (KfTab *)(hp + oTab);
  for (size_t k = 0; k < K; k++) {
    cam[k] = lba::Cam{(double)kf_cam[k].fx, (double)kf_cam[k].fy, (double)kf_cam[k].cx, (double)kf_cam[k].cy, (double)kf_cam[k].bf};
    est0[k] = pose::est_from_pose(kf_Tcw[k].q, kf_Tcw[k].t);  // :1766, :1783
    tab[k].kps = kfs[k]->d_kps, tab[k].ur = kfs[k]->has_uright ? kfs[k]->d_uright : nullptr;  // the pointers as they are NOW
  }
  memcpy(hp + oTcw, kf_Tcw, K * sizeof(vsg_pose_se3));
  memset(hp + oState, 0, sizeof(lba::State));
  *(int32_t *)(hp + oOk2) = 1;
  lba::State *mirror = (lba::State *)(hp + oMirror);
  memset(mirror, 0, sizeof(*mirror));

  lba::Prob p;
  memset(&p, 0, sizeof(p));
  p.K = T.K, p.Ko = T.Ko, p.P = T.P, p.E = T.E, p.n = (int)n, p.nb = (int)nb, p.Ge = (int)Ge, p.Gp = (int)Gp, p.iterations = iterations;
  p.e_kf = (const int32_t *)(dv + oEkf), p.e_pt = (const int32_t *)(dv + oEpt), p.e_opt = (const int32_t *)(dv + oEopt);
  p.p_off = (const int32_t *)(dv + oPoff), p.k_off = (const int32_t *)(dv + oKoff), p.k_edge = (const int32_t *)(dv + oKedge);
  p.b_i = (const int32_t *)(dv + oBi), p.b_j = (const int32_t *)(dv + oBj), p.b_off = (const int32_t *)(dv + oBoff);
  p.pair_a = (const int32_t *)(dv + oPa), p.pair_b = (const int32_t *)(dv + oPb), p.opt_kf = (const int32_t *)(dv + oOptKf);
  p.cam = (const lba::Cam *)(dv + oCam), p.obs = (double *)(dv + dObs), p.w = (double *)(dv + dW), p.flag = dv + dFlag;
  p.est[0] = (lba::Est *)(dv + oEst0), p.est[1] = (lba::Est *)(dv + dEst1), p.X[0] = (double *)(dv + dX0), p.X[1] = (double *)(dv + dX1);
  p.chi2 = (double *)(dv + dChi), p.Hpl = (double *)(dv + dHpl), p.HppC = (double *)(dv + dHppC), p.HllC = (double *)(dv + dHllC);
  p.BDinv = (double *)(dv + dBD), p.c = (double *)(dv + dC), p.Hpp = (double *)(dv + dHpp), p.Hll = (double *)(dv + dHll);
  p.M = (double *)(dv + dM), p.bs = (double *)(dv + dBs), p.xp = (double *)(dv + dXp), p.chiPart = (double *)(dv + dChiPart);
  p.maxPart = (double *)(dv + dMaxPart), p.maxKf = (double *)(dv + dMaxKf), p.scalePart = (double *)(dv + dScale);
  p.ok2 = (int32_t *)(dv + oOk2), p.S = (lba::State *)(dv + oState);
  SetupArgs SA;
  memset(&SA, 0, sizeof(SA));
  SA.tab = (const KfTab *)(dv + oTab), SA.e_idx = (const int32_t *)(dv + oEidx), SA.slots = (const int32_t *)(dv + oSlots), SA.pos = F.pos;
  for (int l = 0; l < 16; l++) SA.sig[l] = inv_level_sigma2[l < nlevels ? l : nlevels - 1];
  FinalArgs FA;
  FA.slots = SA.slots, FA.pos = F.pos, FA.Tcw = (const vsg_pose_se3 *)(dv + oTcw), FA.opt_of = (const int32_t *)(dv + oOptOf);
  FA.erase = dp + oErase, FA.chi2 = (double *)(dp + oChi2), FA.kf_out = (vsg_pose_se3d *)(dp + oKfOut), FA.pos_out = (float *)(dp + oPosOut);
  lba::State *mirror_dev = (lba::State *)(dp + oMirror);

  TRY_HIP(hipMemcpyAsync(dv, hp, in_bytes, hipMemcpyHostToDevice, c->stream));
  // from here on an error waits for the stream before it returns: the arenas belong to the next call
  hipStream_t st = c->stream;
  const dim3 B(lba::kThreads);
  const size_t most = E > P ? (E > K ? E : K) : (P > K ? P : K);
  const unsigned gAll = (unsigned)((most + lba::kThreads - 1) / lba::kThreads);
  const int Gs = (int)((nb + kBlocksPerGroup - 1) / kBlocksPerGroup);
  const int S = t_trial_slots > 0 ? t_trial_slots : (int)kTrialSlots;
  hipLaunchKernelGGL(k_setup, dim3(gAll), B, 0, st, p, SA);
  bool failed = false, stopped = false;
  for (int it = 0; it < iterations && !failed; it++) {
    hipLaunchKernelGGL(k_linearise, dim3((unsigned)Ge), B, 0, st, p, it);
    hipLaunchKernelGGL(k_gather, dim3((unsigned)(Gp + Ko)), B, 0, st, p, it);
    hipLaunchKernelGGL(k_begin, dim3(1), dim3(1), 0, st, p, it, mirror_dev);
    bool closed = false;
    for (int q = 0; q < lba::kTrials && !closed && !failed;) {
      for (int s = 0; s < S && q < lba::kTrials; s++, q++) {
        hipLaunchKernelGGL(k_trial_edges, dim3((unsigned)Ge), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_schur, dim3((unsigned)(Gs + (int)Ko)), B, 0, st, p, it, q, Gs);
        hipLaunchKernelGGL(k_solve, dim3(1), dim3(lba::kSolveThreads), 0, st, p, it, q);
        hipLaunchKernelGGL(k_backsub, dim3((unsigned)(Gp + 1)), B, 0, st, p, it, q);
        hipLaunchKernelGGL(k_error, dim3((unsigned)Ge), B, 0, st, p, it, q);
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
