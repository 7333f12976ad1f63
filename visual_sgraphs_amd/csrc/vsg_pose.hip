// vsg_pose.hip -- Optimizer::PoseOptimization (Optimizer.cc:1063-1452) on a resident frame and resident map points:
// vsg_frame_pose_optimization / vsg_frame_pose_optimization_resume (include/vsg_orb.h).
//
// ONE persistent workgroup of pose::kThreads lanes runs the whole routine (k_pose_optimize): the four rounds are a serial
// chain of evaluations (up to 4 x 10 x 11 of them), each a short pass over the edges followed by a 6x6 solve, so there
// is nothing for a second workgroup to do that would not cost a grid-wide barrier per evaluation.  The call is one
// enqueue and one wait.  The arithmetic is csrc/vsg_pose_opt.h, shared with the host build bit for bit; this file adds
// the gather, the reduction tree on the wavefronts and the copy-out.
//
// Edge data (64 bytes per edge, pose::Edge) stays in a per-frame device buffer and is read from L2 in every pass; the
// accumulators (28 doubles) live in registers and only the four waves' sums cross LDS (DESIGN.md section 8 weighs the
// alternatives).  Edge i is always touched by lane i % kThreads -- gather, every pass, classification, copy-out -- so
// the edge arrays need no ordering between lanes; only the reductions synchronise.  The 6x6 solve and the Levenberg
// state run redundantly on every lane on identical bits, which keeps control flow uniform across the workgroup.
#include <cstring>
#include <vector>

#include "vsg_frame_int.h"
#include "vsg_pose_opt.h"
#include "vsg_track_int.h"

using namespace vsg;

namespace {

struct PoseOut {
  double q[4], t[3];
  int32_t n_bad, rounds_run, held, pad;
};

struct PoseArgs {
  pose::Ctl *ctl;  // the frame's pose buffer: [Ctl | Edge[capacity] | flags[capacity] | chi2[capacity]]
  pose::Edge *edges;
  uint8_t *flags;
  float *chi2;
  const int32_t *feat, *slot;  // per edge, in the pinned arena (kModeAll / kModeHold)
  const uint8_t *removed;      // per edge, in the pinned arena (kModeResume; nullptr: none)
  // a chain call (vsg_track.hip): the status words of the walk kernel in front of this one, {nmatches, n_edges, flags};
  // feat / slot are that kernel's edge list in the device arena and n_edges is status[1].  nullptr: the host's n_edges
  const int32_t *chain;
  const float *pos;            // the store's world positions
  const KeyPointPOD *kps;
  const float *uright;  // nullptr: every feature is monocular
  float inv_sigma2[16];
  pose::Cam cam;
  pose::Est input;
  int n_edges, mode;
  uint8_t *out_flags;  // per edge, pinned
  float *out_chi2;     // per edge, pinned
  PoseOut *out;        // pinned
};

struct DevTeam {
  pose::Cam K;
  pose::Edge *edges;
  uint8_t *flags;
  float *chi2_out;
  int n_edges;
  double *lds;  // [kWaves][kAcc]

  // the fixed tree of vsg_pose_opt.h: butterfly over the wave's 64 lanes, then the waves serially.  The f64 VALU rate and
  // the cost of these 6 x 2 cross-lane moves per value have not been measured on this part.
  __device__ void reduce(double *acc, int n) {
    const int lane = threadIdx.x & (pose::kWave - 1), wave = threadIdx.x / pose::kWave;
    for (int k = 0; k < n; k++) {
      double v = acc[k];
#pragma unroll
      for (int s = 1; s < pose::kWave; s <<= 1) v = v + __shfl_xor(v, s, pose::kWave);
      acc[k] = v;
    }
    __syncthreads();  // the previous reduction's readers are done with lds
    if (lane == 0)
      for (int k = 0; k < n; k++) lds[wave * pose::kAcc + k] = acc[k];
    __syncthreads();
    for (int k = 0; k < n; k++) {
      double t = lds[k];
#pragma unroll
      for (int w = 1; w < pose::kWaves; w++) t = t + lds[w * pose::kAcc + k];
      acc[k] = t;
    }
  }
  __device__ void build(const pose::Est &T, bool robust, double *acc) {
    pose::thread_partial(K, T, edges, flags, n_edges, (int)threadIdx.x, robust, true, acc);
    reduce(acc, pose::kAcc);
  }
  __device__ double chi(const pose::Est &T, bool robust) {
    double c;
    pose::thread_partial(K, T, edges, flags, n_edges, (int)threadIdx.x, robust, false, &c);
    reduce(&c, 1);
    return c;
  }
  __device__ void classify(const pose::Est &T, int *n_bad, int *gone) {
    int nb = 0, ng = 0;
    for (int i = threadIdx.x; i < n_edges; i += pose::kThreads) {
      int g = 0;
      nb += pose::classify_edge(K, T, &edges[i], &flags[i], &chi2_out[i], &g);
      ng += g;
    }
    // integer counts: any order gives the same sums (both fit a double exactly)
    double c[2] = {(double)nb, (double)ng};
    reduce(c, 2);
    *n_bad += (int)c[0], *gone += (int)c[1];
  }
};

__global__ __launch_bounds__(pose::kThreads) void k_pose_optimize(PoseArgs A) {
  __shared__ double lds[pose::kWaves * pose::kAcc];
  __shared__ pose::Ctl ctl;
  const int tid = threadIdx.x, E = A.chain ? A.chain[1] : A.n_edges;
  if (A.chain && A.chain[2] != 0) {
    // the lists overflowed, the search found fewer than 20 matches or there are fewer than 3 edges: the header alone
    if (tid == 0) {
      PoseOut o;
      for (int k = 0; k < 4; k++) o.q[k] = A.input.q[k];
      for (int k = 0; k < 3; k++) o.t[k] = A.input.t[k];
      o.n_bad = 0, o.rounds_run = 0, o.held = 0, o.pad = 0;
      *A.out = o;
    }
    return;
  }
  if (A.mode == pose::kModeResume) {
    // round 2's plane step on the host (:1270-1335): mvpMapPoints[j] = NULL, mvbOutlier[j] = true
    if (A.removed)
      for (int i = tid; i < E; i += pose::kThreads)
        if (A.removed[i]) A.flags[i] = (uint8_t)(A.flags[i] | pose::kOutlier | pose::kRemoved);
    if (tid == 0) ctl = *A.ctl;
  } else {
    // the edges in feature order (:1109-1180): GetWorldPos().cast<double>(), kpUn.pt, mvuRight, mvInvLevelSigma2[octave]
    for (int i = tid; i < E; i += pose::kThreads) {
      const int f = A.feat[i], s = A.slot[i];
      const KeyPointPOD kp = A.kps[f];
      const float ur = A.uright ? A.uright[f] : -1.0f;
      const bool stereo = !(ur < 0);  // if (pFrame->mvuRight[i] < 0) monocular
      pose::Edge e;
      e.X[0] = (double)A.pos[3 * (size_t)s], e.X[1] = (double)A.pos[3 * (size_t)s + 1], e.X[2] = (double)A.pos[3 * (size_t)s + 2];
      e.obs[0] = (double)kp.x, e.obs[1] = (double)kp.y, e.obs[2] = stereo ? (double)ur : 0.0;
      e.w = (double)A.inv_sigma2[kp.octave & 15];
      e.chi2 = 0.0;
      A.edges[i] = e;
      A.flags[i] = stereo ? pose::kStereo : 0;  // mvbOutlier[i] = false
      A.chi2[i] = 0.0f;
    }
    if (tid == 0) {
      ctl.cam = A.cam, ctl.input = A.input, ctl.n_edges = E;
    }
  }
  __syncthreads();
  pose::Ctl C = ctl;  // every lane carries the same state
  DevTeam tm = {C.cam, A.edges, A.flags, A.chi2, E, lds};
  pose::run_rounds(tm, &C, A.mode);
  for (int i = tid; i < E; i += pose::kThreads) {
    A.out_flags[i] = A.flags[i];
    A.out_chi2[i] = A.chi2[i];
  }
  if (tid == 0) {
    *A.ctl = C;
    PoseOut o;
    for (int k = 0; k < 4; k++) o.q[k] = pose::canon(C.est.q[k]);
    for (int k = 0; k < 3; k++) o.t[k] = pose::canon(C.est.t[k]);
    o.n_bad = C.n_bad, o.rounds_run = C.rounds_run, o.held = C.held, o.pad = 0;
    *A.out = o;
  }
}

struct PoseLayout {
  size_t oCtl, oEdges, oFlags, oChi2, total;
  explicit PoseLayout(size_t cap) {
    Stage st;
    oCtl = st.add(sizeof(pose::Ctl)), oEdges = st.add(cap * sizeof(pose::Edge)), oFlags = st.add(cap), oChi2 = st.add(cap * 4);
    total = st.total;
  }
};

void fill_result(vsg_pose_result *res, const double *q, const double *t, int n_initial, int n_bad, int rounds, int held) {
  for (int k = 0; k < 4; k++) res->q[k] = q[k];
  for (int k = 0; k < 3; k++) res->t[k] = t[k];
  res->n_initial = n_initial, res->n_bad = n_bad, res->rounds_run = rounds, res->held = held;
}

// enqueue, wait, copy out: what the call and its resume share.  The staging [feat | slot | removed] has been written.
int run_pose(vsg_frame *F, ThreadCtx *c, PoseArgs &A, size_t oOutFlags, size_t oOutChi2, size_t oOut, uint8_t *outlier,
             float *chi2, vsg_pose_result *res) {
  const PoseLayout L((size_t)F->capacity);
  A.ctl = (pose::Ctl *)(F->d_pose + L.oCtl), A.edges = (pose::Edge *)(F->d_pose + L.oEdges);
  A.flags = F->d_pose + L.oFlags, A.chi2 = (float *)(F->d_pose + L.oChi2);
  A.out_flags = c->d_pin + oOutFlags, A.out_chi2 = (float *)(c->d_pin + oOutChi2), A.out = (PoseOut *)(c->d_pin + oOut);
  hipLaunchKernelGGL(k_pose_optimize, dim3(1), dim3(pose::kThreads), 0, c->stream, A);
  const hipError_t e1 = hipGetLastError(), e2 = hipStreamSynchronize(c->stream);
  if (e1 != hipSuccess || e2 != hipSuccess) return VSG_ERR_HIP;
  const PoseOut *o = (const PoseOut *)(c->h_pin + oOut);
  const uint8_t *fl = c->h_pin + oOutFlags;
  const float *ch = (const float *)(c->h_pin + oOutChi2);
  const int E = A.n_edges;
  for (int e = 0; e < E; e++) {
    const int i = F->pose_feat[(size_t)e];
    outlier[i] = (fl[e] & pose::kOutlier) ? 1 : 0;
    if (chi2) chi2[i] = ch[e];
  }
  fill_result(res, o->q, o->t, E, o->n_bad, o->rounds_run, o->held);
  F->pose_held = o->held != 0;
  return o->held ? 0 : E - o->n_bad;
}

}  // namespace

namespace vsg {

size_t pose_chain_bytes(int nf) {
  const size_t N = (size_t)(nf > 0 ? nf : 1);
  Stage st;
  st.add(N), st.add(N * 4), st.add(sizeof(PoseOut));
  return st.total;
}

int pose_chain_enqueue(vsg_frame *F, ThreadCtx *c, const StoreView &S, const int32_t *d_edge_feat,
                       const int32_t *d_edge_slot, const int32_t *d_status, const vsg_pose_se3 *Tcw,
                       const vsg_frame_pose *cam, const float *inv_level_sigma2, int nlevels, int hold_round,
                       size_t pin_base) {
  if (!F->d_pose) {  // allocated on first use, freed with the frame
    const PoseLayout L((size_t)F->capacity);
    TRY_HIP(hipMalloc((void **)&F->d_pose, L.total));
  }
  const size_t N = (size_t)(F->n > 0 ? F->n : 1);
  Stage st;
  const size_t oOutFlags = pin_base + st.add(N), oOutChi2 = pin_base + st.add(N * 4), oOut = pin_base + st.add(sizeof(PoseOut));
  PoseArgs A;
  memset(&A, 0, sizeof(A));
  A.feat = d_edge_feat, A.slot = d_edge_slot, A.chain = d_status;
  A.pos = S.pos, A.kps = F->d_kps, A.uright = F->has_uright ? F->d_uright : nullptr;
  for (int l = 0; l < 16; l++) A.inv_sigma2[l] = inv_level_sigma2[l < nlevels ? l : nlevels - 1];
  A.cam = {(double)cam->fx, (double)cam->fy, (double)cam->cx, (double)cam->cy, (double)cam->mbf};
  A.input = pose::est_from_pose(Tcw->q, Tcw->t);
  A.n_edges = 0, A.mode = hold_round == 2 ? pose::kModeHold : pose::kModeAll;
  const PoseLayout L((size_t)F->capacity);
  A.ctl = (pose::Ctl *)(F->d_pose + L.oCtl), A.edges = (pose::Edge *)(F->d_pose + L.oEdges);
  A.flags = F->d_pose + L.oFlags, A.chi2 = (float *)(F->d_pose + L.oChi2);
  A.out_flags = c->d_pin + oOutFlags, A.out_chi2 = (float *)(c->d_pin + oOutChi2), A.out = (PoseOut *)(c->d_pin + oOut);
  F->pose_held = false;
  hipLaunchKernelGGL(k_pose_optimize, dim3(1), dim3(pose::kThreads), 0, c->stream, A);
  return hipGetLastError() == hipSuccess ? VSG_OK : VSG_ERR_HIP;
}

int pose_chain_finish(vsg_frame *F, ThreadCtx *c, size_t pin_base, const int32_t *h_edge_feat, int n_edges,
                      uint8_t *outlier, float *chi2, vsg_pose_result *res) {
  const size_t N = (size_t)(F->n > 0 ? F->n : 1);
  Stage st;
  const size_t oOutFlags = pin_base + st.add(N), oOutChi2 = pin_base + st.add(N * 4), oOut = pin_base + st.add(sizeof(PoseOut));
  const PoseOut *o = (const PoseOut *)(c->h_pin + oOut);
  const uint8_t *fl = c->h_pin + oOutFlags;
  const float *ch = (const float *)(c->h_pin + oOutChi2);
  F->pose_feat.assign(h_edge_feat, h_edge_feat + n_edges);  // what _resume maps its edges through
  for (int e = 0; e < n_edges; e++) {
    const int i = h_edge_feat[e];
    outlier[i] = (fl[e] & pose::kOutlier) ? 1 : 0;
    if (chi2) chi2[i] = ch[e];
  }
  fill_result(res, o->q, o->t, n_edges, o->n_bad, o->rounds_run, o->held);
  F->pose_held = o->held != 0;
  return o->held ? 0 : n_edges - o->n_bad;
}

void pose_result_input(const vsg_pose_se3 *Tcw, int n_edges, vsg_pose_result *res) {
  const pose::Est input = pose::est_from_pose(Tcw->q, Tcw->t);
  fill_result(res, input.q, input.t, n_edges, 0, 0, 0);
}

}  // namespace vsg

extern "C" {

int vsg_frame_pose_optimization(vsg_frame *F, vsg_mappoints *mp, const int32_t *feat_slots, const vsg_pose_se3 *Tcw,
                                float fx, float fy, float cx, float cy, float bf, const float *inv_level_sigma2,
                                int nlevels, int hold_round, uint8_t *outlier, float *chi2, vsg_pose_result *res) {
  StoreView S;
  if (!F || !F->d_block || !store_view(mp, &S) || !feat_slots || !Tcw || !inv_level_sigma2 || !res || !outlier)
    return VSG_ERR_INVALID;
  if (nlevels < 1 || nlevels > 16 || (hold_round != -1 && hold_round != 2)) return VSG_ERR_INVALID;
  if (F->nleft != -1) return VSG_ERR_UNSUPPORTED;  // EdgeSE3ProjectXYZOnlyPoseToBody, KannalaBrandt8 (:1182-1246)
  if (F->device != S.device) return VSG_ERR_INVALID;
  const int n = F->n;
  int E = 0;
  if (!pose::check_slots(n, feat_slots, S.capacity, nlevels, (int)F->h_kps.size(),
                         [&](int i) { return F->h_kps[(size_t)i].octave; }, &E))
    return VSG_ERR_INVALID;
  // everything the kernel indexes has been bounded; nothing has been enqueued
  const pose::Est input = pose::est_from_pose(Tcw->q, Tcw->t);
  F->pose_held = false;
  if (E < 3) {  // :1251; mvbOutlier[i] = false has happened for every feature with a map point (:1121, :1149)
    for (int i = 0; i < n; i++)
      if (feat_slots[i] >= 0) outlier[i] = 0;
    fill_result(res, input.q, input.t, E, 0, 0, 0);
    return 0;
  }
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(F->device, &rc);
  if (!c) return rc;
  if (!F->d_pose) {  // allocated on first use, freed with the frame
    const PoseLayout L((size_t)F->capacity);
    TRY_HIP(hipMalloc((void **)&F->d_pose, L.total));
  }
  const size_t N = (size_t)E;
  Stage st;
  const size_t oFeat = st.add(N * 4), oSlot = st.add(N * 4), oOutFlags = st.add(N), oOutChi2 = st.add(N * 4),
               oOut = st.add(sizeof(PoseOut));
  rc = ctx_reserve(c, st.total, 0);
  if (rc != VSG_OK) return rc;
  int32_t *hf = (int32_t *)(c->h_pin + oFeat), *hs = (int32_t *)(c->h_pin + oSlot);
  F->pose_feat.resize(N);
  for (int i = 0, e = 0; i < n; i++)
    if (feat_slots[i] >= 0) hf[e] = i, hs[e] = feat_slots[i], F->pose_feat[(size_t)e] = i, e++;
  PoseArgs A;
  memset(&A, 0, sizeof(A));
  A.feat = (const int32_t *)(c->d_pin + oFeat), A.slot = (const int32_t *)(c->d_pin + oSlot);
  A.pos = S.pos, A.kps = F->d_kps, A.uright = F->has_uright ? F->d_uright : nullptr;
  for (int l = 0; l < 16; l++) A.inv_sigma2[l] = inv_level_sigma2[l < nlevels ? l : nlevels - 1];
  A.cam = {(double)fx, (double)fy, (double)cx, (double)cy, (double)bf};
  A.input = input;
  A.n_edges = E, A.mode = hold_round == 2 ? pose::kModeHold : pose::kModeAll;
  return run_pose(F, c, A, oOutFlags, oOutChi2, oOut, outlier, chi2, res);
}

int vsg_frame_pose_optimization_resume(vsg_frame *F, const uint8_t *removed, uint8_t *outlier, float *chi2,
                                       vsg_pose_result *res) {
  if (!F || !F->d_block || !outlier || !res) return VSG_ERR_INVALID;
  if (!F->pose_held || !F->d_pose) return VSG_ERR_INVALID;  // nothing held, features rewritten since, or resumed before
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(F->device, &rc);
  if (!c) return rc;
  const size_t N = F->pose_feat.size();
  Stage st;
  const size_t oRem = st.add(N), oOutFlags = st.add(N), oOutChi2 = st.add(N * 4), oOut = st.add(sizeof(PoseOut));
  rc = ctx_reserve(c, st.total, 0);
  if (rc != VSG_OK) return rc;
  F->pose_held = false;
  if (removed)
    for (size_t e = 0; e < N; e++) c->h_pin[oRem + e] = removed[F->pose_feat[e]] ? 1 : 0;
  PoseArgs A;
  memset(&A, 0, sizeof(A));
  A.removed = removed ? c->d_pin + oRem : nullptr;
  A.n_edges = (int)N, A.mode = pose::kModeResume;
  return run_pose(F, c, A, oOutFlags, oOutChi2, oOut, outlier, chi2, res);
}

}  // extern "C"
