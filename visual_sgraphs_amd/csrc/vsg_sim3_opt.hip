// vsg_sim3_opt.hip -- Optimizer::OptimizeSim3 (Optimizer.cc:3261-3529) on two resident keyframes and resident map points:
// vsg_frame_optimize_sim3 (include/vsg_orb.h).
//
// ONE persistent workgroup of sim3opt::kThreads lanes runs the whole routine (k_sim3_optimize), as k_pose_optimize does
// and for the same reason: the two optimisations are a serial chain of evaluations (up to 15 iterations of at most 11
// each), every one a short pass over the pairs followed by a 7x7 solve.  One enqueue, one wait.  The arithmetic is
// csrc/vsg_sim3_opt.h, shared with the host build bit for bit; this file adds the gather through both stores and both
// keyframes' resident keypoints, the reduction tree on the wavefronts and the copy-out.
//
// THE PERTURBED ESTIMATES of the numeric Jacobian (14 of them and their inverses, 28 x 64 bytes) are computed by lanes
// 0 .. 13, one each, at the head of every build pass and shared through LDS; every lane reads them from there, so they
// cost no registers.  The host's Team computes the same 14 with the same function.  The reduction's barriers separate one
// pass's readers from the next pass's writers (every build is followed by at least one trial's reduction).
//
// Pair data (112 bytes per candidate, sim3opt::Pair) and the states live in the CALLING THREAD's device arena, not in a
// buffer of a frame or a store: two threads may optimise on the same stores and keyframes at once.  Pair p is always
// touched by lane p % kThreads -- gather, every pass, both checks, copy-out -- so the pair arrays need no ordering between
// lanes; only the reductions synchronise.  The 7x7 solve and the Levenberg state run redundantly on every lane on
// identical bits, which keeps control flow uniform across the workgroup.  All stores are plain vector stores.
#include <cstring>

#include "vsg_frame_int.h"
#include "vsg_sim3_opt.h"

using namespace vsg;

namespace {

struct OptOut {
  vsg_sim3d S12;
  int32_t n_correspondences, n_bad, n_in, n_in_kf2, n_out_kf2, more_iterations, updated, ret;
};

struct OptArgs {
  const float *pos1, *pos2;  // the stores' GetWorldPos()
  const KeyPointPOD *kps1, *kps2;
  const int32_t *feat, *slot1, *slot2, *idx2, *level2;  // per candidate, in the pinned arena
  vsg_frame_pose kf1, kf2;
  float sig1[16], sig2[16];
  sim3opt::Sim3 input;
  double th2, delta;
  int n_pairs, fix_scale, all_points;
  sim3opt::Pair *pairs;  // [n_pairs], device arena
  uint8_t *state;        // [n_pairs], device arena
  uint8_t *out_state;    // [n_pairs], pinned
  double *out_chi2;      // [2 n_pairs], pinned
  OptOut *out;           // pinned
};

struct DevTeam {
  sim3opt::Cams K;
  sim3opt::Pair *pairs;
  uint8_t *state;
  int n_pairs;
  double delta;
  bool fix_scale;
  double *lds;          // [kWaves][kAcc]
  sim3opt::Pert *pert;  // LDS

  // the fixed tree of vsg_pose_opt.h: butterfly over the wave's 64 lanes, then the waves serially
  template <int N>
  __device__ __forceinline__ void reduce(double *acc) {
    const int lane = threadIdx.x & (pose::kWave - 1), wave = threadIdx.x / pose::kWave;
#pragma unroll
    for (int k = 0; k < N; k++) {
      double v = acc[k];
#pragma unroll
      for (int s = 1; s < pose::kWave; s <<= 1) v = v + __shfl_xor(v, s, pose::kWave);
      acc[k] = v;
    }
    __syncthreads();  // the previous reduction's readers are done with lds
    if (lane == 0) {
#pragma unroll
      for (int k = 0; k < N; k++) lds[wave * sim3opt::kAcc + k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; k++) {
      double t = lds[k];
#pragma unroll
      for (int w = 1; w < pose::kWaves; w++) t = t + lds[w * sim3opt::kAcc + k];
      acc[k] = t;
    }
  }
  __device__ void build(const sim3opt::Sim3 &S, bool robust, double *acc) {
    const int tid = (int)threadIdx.x;
    // the last pass that read pert ended before the barriers of the reductions since
    if (tid < sim3opt::kPert) sim3opt::perturbed(S, tid, fix_scale, &pert->fwd[tid], &pert->inv[tid]);
    __syncthreads();
    sim3opt::thread_partial<true>(K, S, pert, pairs, state, n_pairs, tid, robust, delta, acc);
    reduce<sim3opt::kAcc>(acc);
  }
  __device__ double chi(const sim3opt::Sim3 &S, bool robust) {
    double c;
    sim3opt::thread_partial<false>(K, S, pert, pairs, state, n_pairs, (int)threadIdx.x, robust, delta, &c);
    reduce<1>(&c);
    return c;
  }
  __device__ int check(const sim3opt::Sim3 &S, double th2, bool fresh, int bad_state) {
    const sim3opt::Sim3 Sinv = sim3opt::sim3_inverse(S);
    int bad = 0;
    for (int p = threadIdx.x; p < n_pairs; p += sim3opt::kThreads)
      bad += sim3opt::check_pair(K, S, Sinv, &pairs[p], &state[p], th2, fresh, bad_state);
    double c = (double)bad;  // an integer count: any order gives the same sum
    reduce<1>(&c);
    return (int)c;
  }
};

__global__ __launch_bounds__(sim3opt::kThreads) void k_sim3_optimize(OptArgs A) {
  __shared__ double lds[pose::kWaves * sim3opt::kAcc];
  __shared__ sim3opt::Pert pert;
  const int tid = threadIdx.x, N = A.n_pairs;
  DevTeam tm = {sim3opt::cams_of(A.kf1, A.kf2), A.pairs, A.state, N, A.delta, A.fix_scale != 0, lds, &pert};
  // the pair set-up (:3313-3450) for the candidates in feature order; every index was bounded by the host
  int n_corr = 0, n_in2 = 0, n_out2 = 0;
  for (int p = tid; p < N; p += sim3opt::kThreads) {
    const int f = A.feat[p], i2 = A.idx2[p];
    const size_t s1 = (size_t)A.slot1[p], s2 = (size_t)A.slot2[p];
    const KeyPointPOD k1 = A.kps1[f];
    float k2x = 0.0f, k2y = 0.0f;
    int o2 = A.level2[p];
    if (i2 >= 0) {
      const KeyPointPOD k2 = A.kps2[i2];
      k2x = k2.x, k2y = k2.y, o2 = k2.octave;
    }
    const float X1[3] = {A.pos1[3 * s1], A.pos1[3 * s1 + 1], A.pos1[3 * s1 + 2]};
    const float X2[3] = {A.pos2[3 * s2], A.pos2[3 * s2 + 1], A.pos2[3 * s2 + 2]};
    sim3opt::Pair P;
    memset(&P, 0, sizeof(P));
    const int st = sim3opt::make_pair(A.kf1, A.kf2, X1, X2, k1.x, k1.y, k1.octave, i2, k2x, k2y, o2, A.sig1, A.sig2,
                                      A.all_points != 0, &P);
    A.pairs[p] = P;
    A.state[p] = (uint8_t)st;
    if (st == sim3opt::kInlier) n_corr++, (i2 >= 0 ? n_in2 : n_out2)++;
  }
  double cnt[3] = {(double)n_corr, (double)n_in2, (double)n_out2};  // integer counts: exact in any order
  tm.reduce<3>(cnt);
  const sim3opt::Outcome o = sim3opt::run(tm, A.input, (int)cnt[0], A.th2, A.fix_scale != 0);
  for (int p = tid; p < N; p += sim3opt::kThreads) {
    A.out_state[p] = A.state[p];
    A.out_chi2[2 * (size_t)p] = pose::canon(A.pairs[p].chi12);
    A.out_chi2[2 * (size_t)p + 1] = pose::canon(A.pairs[p].chi21);
  }
  if (tid == 0) {
    OptOut r;
    r.S12 = sim3opt::sim3d_canon(o.S12);
    r.n_correspondences = (int)cnt[0], r.n_in_kf2 = (int)cnt[1], r.n_out_kf2 = (int)cnt[2];
    r.n_bad = o.n_bad, r.n_in = o.n_in, r.more_iterations = o.more_iterations, r.updated = o.updated, r.ret = o.ret;
    *A.out = r;
  }
}

}  // namespace

extern "C" {

int vsg_frame_optimize_sim3(vsg_frame *kf1, vsg_frame *kf2, vsg_mappoints *mp1, vsg_mappoints *mp2, const int32_t *slots1,
                            const int32_t *slots2, const int32_t *idx2, const int32_t *level2, const vsg_frame_pose *pose1,
                            const vsg_frame_pose *pose2, const float *inv_level_sigma2_1, const float *inv_level_sigma2_2,
                            int nlevels, const vsg_sim3d *S12, float th2, int fix_scale, int all_points, uint8_t *state,
                            double *chi2, vsg_sim3_opt_result *res) {
  StoreView S1, S2;
  if (!kf1 || !kf1->d_block || !kf2 || !kf2->d_block || !store_view(mp1, &S1) || !store_view(mp2, &S2)) return VSG_ERR_INVALID;
  if (!slots1 || !slots2 || !idx2 || !level2 || !pose1 || !pose2 || !inv_level_sigma2_1 || !inv_level_sigma2_2 || !S12 ||
      !state || !res)
    return VSG_ERR_INVALID;
  if (nlevels < 1 || nlevels > 16 || !sim3opt::th2_ok(th2)) return VSG_ERR_INVALID;
  if (kf1->nleft != -1 || kf2->nleft != -1) return VSG_ERR_UNSUPPORTED;  // pCamera2, KannalaBrandt8
  if (kf1->device != kf2->device || kf1->device != S1.device || kf1->device != S2.device) return VSG_ERR_INVALID;
  const int n = kf1->n;
  int n_cand = 0;
  // a frame without its host mirror cannot have its octaves checked here: the kernel masks them to the 16-entry tables
  if (!sim3opt::check_entries(
          n, slots1, slots2, idx2, level2, S1.capacity, S2.capacity, kf2->n, nlevels, all_points != 0,
          [&](int i) { return (size_t)i < kf1->h_kps.size() ? (int)kf1->h_kps[(size_t)i].octave : 0; },
          [&](int i) { return (size_t)i < kf2->h_kps.size() ? (int)kf2->h_kps[(size_t)i].octave : 0; }, &n_cand))
    return VSG_ERR_INVALID;
  // everything the kernel indexes has been bounded; nothing has been enqueued
  if (n_cand == 0) {  // no vertex but the Sim3: optimize() does nothing, nCorrespondences - nBad = 0 < 10 (:3494)
    for (int i = 0; i < n; i++) state[i] = sim3opt::kNoEdge;
    sim3opt::fill_result(res, *S12, sim3opt::Counts{0, 0, 0}, 0, 0, 5, 0);
    return 0;
  }
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(kf1->device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n_cand;
  Stage st;
  const size_t oFeat = st.add(N * 4), oS1 = st.add(N * 4), oS2 = st.add(N * 4), oI2 = st.add(N * 4), oL2 = st.add(N * 4),
               oState = st.add(N), oChi2 = st.add(N * 16), oOut = st.add(sizeof(OptOut));
  const size_t dev_pairs = (N * sizeof(sim3opt::Pair) + 63) & ~(size_t)63;
  rc = ctx_reserve(c, st.total, dev_pairs + N);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_pin;
  int32_t *hf = (int32_t *)(h + oFeat), *h1 = (int32_t *)(h + oS1), *h2 = (int32_t *)(h + oS2), *hi = (int32_t *)(h + oI2),
          *hl = (int32_t *)(h + oL2);
  for (int i = 0, p = 0; i < n; i++)
    if (slots1[i] >= 0 && slots2[i] >= 0) hf[p] = i, h1[p] = slots1[i], h2[p] = slots2[i], hi[p] = idx2[i], hl[p] = level2[i], p++;
  OptArgs A;
  memset(&A, 0, sizeof(A));
  A.pos1 = S1.pos, A.pos2 = S2.pos, A.kps1 = kf1->d_kps, A.kps2 = kf2->d_kps;
  A.feat = (const int32_t *)(d + oFeat), A.slot1 = (const int32_t *)(d + oS1), A.slot2 = (const int32_t *)(d + oS2);
  A.idx2 = (const int32_t *)(d + oI2), A.level2 = (const int32_t *)(d + oL2);
  A.kf1 = *pose1, A.kf2 = *pose2;
  for (int l = 0; l < 16; l++)
    A.sig1[l] = inv_level_sigma2_1[l < nlevels ? l : nlevels - 1], A.sig2[l] = inv_level_sigma2_2[l < nlevels ? l : nlevels - 1];
  A.input = sim3opt::sim3_of(*S12);
  A.th2 = (double)th2, A.delta = sim3opt::huber_delta_of(th2);
  A.n_pairs = n_cand, A.fix_scale = fix_scale ? 1 : 0, A.all_points = all_points ? 1 : 0;
  A.pairs = (sim3opt::Pair *)c->d_buf, A.state = c->d_buf + dev_pairs;
  A.out_state = d + oState, A.out_chi2 = (double *)(d + oChi2), A.out = (OptOut *)(d + oOut);
  hipLaunchKernelGGL(k_sim3_optimize, dim3(1), dim3(sim3opt::kThreads), 0, c->stream, A);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  const OptOut *o = (const OptOut *)(h + oOut);
  const uint8_t *hs = h + oState;
  const double *hc = (const double *)(h + oChi2);
  for (int i = 0; i < n; i++) state[i] = sim3opt::kNoEdge;
  for (size_t p = 0; p < N; p++) {
    const size_t i = (size_t)hf[p];
    state[i] = hs[p];
    if (chi2 && hs[p] >= sim3opt::kInlier && hs[p] <= sim3opt::kBadSecond) chi2[2 * i] = hc[2 * p], chi2[2 * i + 1] = hc[2 * p + 1];
  }
  const sim3opt::Counts cn = {o->n_correspondences, o->n_in_kf2, o->n_out_kf2};
  // a call that returned before :3526 leaves g2oS12 alone: the caller's bytes, not a canonical copy of them
  sim3opt::fill_result(res, o->updated ? o->S12 : *S12, cn, o->n_bad, o->n_in, o->more_iterations, o->updated);
  return o->ret;
}

}  // extern "C"
