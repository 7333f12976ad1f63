// vsg_track.hip -- Tracking::TrackWithMotionModel (Tracking.cc:2945-3005) as ONE enqueue and ONE wait:
// vsg_frame_track_with_motion_model (include/vsg_orb.h).
//
//   projection kernel -> k_window_search -> k_track_walk -> k_pose_optimize          (one stream, no host step between)
//
// The first two are the resident searches' own (vsg_mappoints.hip, vsg_window.hip) with the candidate lists left in the
// device arena; the last is Optimizer::PoseOptimization (vsg_pose.hip) reading its edges from the buffer k_track_walk
// wrote.  k_track_walk is what used to be the host's ordered pass (vsg_walks.h) between two waits: ONE workgroup runs
// csrc/vsg_walks_dev.h -- rounds to the fixed point of "a feature is blocked for q iff it was blocked on entry or an
// observed point q' < q claimed it", the last-writer rule, the rotation filter on claims, the per-feature slots and the
// edge list in feature order -- with the per-feature and per-query state in LDS.  It sits IN FRONT of the optimisation,
// not inside it: k_pose_optimize already runs at its register limit.  The matches never leave the device between the
// search and the solve; the host reads them once, after the wait, together with the pose.
//
// Tracking::TrackLocalMap (Tracking.cc:3019-3131) is the same chain behind k_frustum: vsg_frame_track_local_map.  The walk
// runs in its local form (q_valid = mbTrackInView, the ratio test) and is given the features' slots on entry instead of a
// blocked array: k_track_walk's prologue derives "blocked on entry" from them and the store's observed flags, and
// walkdev::run keeps the entry slot of every feature nobody claims.  The statistics loop that ends the routine runs on the
// host after the wait (vsg_track_stats.h).
#include <cstring>
#include <vector>

#include "../../include/vsg_orb_debug.h"
#include "vsg_track_int.h"
#include "vsg_track_stats.h"
#include "vsg_walks_dev.h"

using namespace vsg;

namespace {

// kWalkLdsMax: what one workgroup may take of LDS without raising the function's limit, static part included.  The cap is
// this file's choice, not the part's (a CU of gfx950 has 160 KB): a frame and a last frame with 2 nf + nq above about
// 16000 are refused with VSG_ERR_CAPACITY.
enum { kWalkThreads = 1024, kWalkWaves = kWalkThreads / 64, kWalkStaticLds = kWalkWaves * 4, kWalkLdsMax = 64 * 1024 };

struct DevTeam {
  int *wsum;  // [kWalkWaves], LDS
  template <class F>
  __device__ void each(int n, F f) {
    for (int i = threadIdx.x; i < n; i += kWalkThreads) f(i);
    __syncthreads();
  }
  __device__ void amin(int32_t *p, int v) { atomicMin(p, v); }
  __device__ void amax(int32_t *p, int v) { atomicMax(p, v); }
  __device__ void aadd(int32_t *p, int v) { atomicAdd(p, v); }
  // positions in ascending i: a ballot inside the wave, the waves' counts through LDS, kWalkThreads items at a time
  template <class P, class E>
  __device__ int compact(int n, P pred, E emit) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += kWalkThreads) {
      const int i = i0 + (int)threadIdx.x;
      const bool p = i < n && pred(i);
      const unsigned long long m = __ballot(p);
      if (lane == 0) wsum[wave] = __popcll(m);
      __syncthreads();
      int before = __popcll(m & ((1ull << lane) - 1ull)), total = 0;
      for (int w = 0; w < kWalkWaves; w++) {
        const int s = wsum[w];
        before += w < wave ? s : 0;
        total += s;
      }
      if (p) emit(i, base + before);
      base += total;
      __syncthreads();
    }
    return base;
  }
};

// LDS: [claim nf | tm nf | choice nq | scratch] as int32, then the bytes [observed nq | q_valid nq | blocked nf]: the flags
// the rounds read again and again are fetched from the pinned arena once.
__host__ __device__ inline size_t walk_lds_bytes(int nq, int nf) {
  return ((size_t)2 * nf + nq + walkdev::kScratchInts) * 4 + (size_t)2 * nq + nf;
}

__global__ __launch_bounds__(kWalkThreads) void k_track_walk(walkdev::Args A) {
  extern __shared__ int32_t lds[];
  __shared__ int wsum[kWalkWaves];
  A.claim = lds, A.tm = lds + A.nf, A.choice = lds + 2 * A.nf, A.scratch = lds + 2 * A.nf + A.nq;
  uint8_t *b_obs = (uint8_t *)(A.scratch + walkdev::kScratchInts), *b_valid = b_obs + A.nq, *b_blk = b_valid + A.nq;
  for (int q = threadIdx.x; q < A.nq; q += kWalkThreads) {
    b_obs[q] = A.observed ? A.observed[q] : 0;
    b_valid[q] = A.q_valid ? A.q_valid[q] : 1;
  }
  // Without a blocked array but with the features' entry slots (the local-map form): a feature is blocked on entry iff
  // its point is observed (ORBmatcher.cc:86-88).  The host bounded every slot by the store's capacity.
  const bool from_slots = !A.blocked_in && A.slots_in && A.slot_observed;
  for (int i = threadIdx.x; i < A.nf; i += kWalkThreads) {
    uint8_t b = A.blocked_in ? A.blocked_in[i] : 0;
    if (from_slots) {
      const int s = A.slots_in[i];
      b = s >= 0 ? A.slot_observed[s] : 0;
    }
    b_blk[i] = b;
  }
  A.observed = b_obs, A.q_valid = b_valid, A.blocked_in = b_blk;
  __syncthreads();
  DevTeam T = {wsum};
  walkdev::run(T, A);
}

// Does a walk of this shape ask for more LDS than kWalkLdsMax?  The refusal of the two chain calls and of the test hook.
inline bool walk_over_cap(int nq, int nf) { return walk_lds_bytes(nq, nf) + kWalkStaticLds > kWalkLdsMax; }

// The one launch of k_track_walk: one workgroup, its LDS sized by the shape.  The chain calls and the test hook
// (vsg_debug_track_walk) enqueue it here and nowhere else.
int walk_launch(hipStream_t stream, const walkdev::Args &A) {
  hipLaunchKernelGGL(k_track_walk, dim3(1), dim3(kWalkThreads), walk_lds_bytes(A.nq, A.nf), stream, A);
  return hipGetLastError() == hipSuccess ? VSG_OK : VSG_ERR_HIP;
}

// The caller's block of a chain call behind the search's blocks.  Pinned: what the host reads after the wait.  Device: the
// edge list and the status.
struct TrackLayout {
  size_t pTm, pTb, pFs, pFo, pStatus, pPose, pSlotsIn, pin_total;
  size_t dFeat, dSlot, dStatus, dev_total;
  // entry_slots: room for the features' slots on entry (the local-map form sends them; the walk reads them)
  explicit TrackLayout(int nf, bool entry_slots = false) {
    const size_t N = (size_t)(nf > 0 ? nf : 1);
    Stage sp;
    pTm = sp.add(N * 4), pTb = sp.add(N), pFs = sp.add(N * 4), pFo = sp.add(N), pStatus = sp.add(sizeof(walkdev::Status));
    pPose = sp.add(pose_chain_bytes(nf));
    pSlotsIn = sp.add(entry_slots ? N * 4 : 0);
    pin_total = sp.total;
    Stage sd;
    dFeat = sd.add(N * 4), dSlot = sd.add(N * 4), dStatus = sd.add(sizeof(walkdev::Status));
    dev_total = sd.total;
  }
};

// k_track_walk behind the search's two kernels, k_pose_optimize behind it, then the call's one wait and the overflow
// accounting of WindowCall::finish from the sum the walk kernel took.  VSG_RETRY: the lists overflowed, nothing was solved.
int walk_solve_wait(TrackSearch &T, const TrackLayout &L, walkdev::Args &A, vsg_frame *F, const StoreView &S,
                    const vsg_pose_se3 *Tcw, const vsg_frame_pose *cam, const float *inv_level_sigma2, int nlevels,
                    int hold_round, walkdev::Status *st) {
  ThreadCtx *c = T.c;
  uint8_t *hp = c->h_pin + T.pin_extra, *dp = c->d_pin + T.pin_extra, *dv = c->d_buf + T.dev_extra;
  A.inline_len = kWinInline, A.cap = T.wc.cap, A.list_total = T.list_total;
  A.ent = T.d_ent, A.off = T.d_off, A.cnt = T.d_cnt;
  A.train_match = (int32_t *)(dp + L.pTm), A.train_blocked = dp + L.pTb, A.feat_slots = (int32_t *)(dp + L.pFs);
  A.feat_observed = dp + L.pFo;
  A.edge_feat = (int32_t *)(dv + L.dFeat), A.edge_slot = (int32_t *)(dv + L.dSlot);
  A.status = (walkdev::Status *)(dv + L.dStatus), A.status2 = (walkdev::Status *)(dp + L.pStatus);
  const int launched = walk_launch(c->stream, A);
  int rc = launched;
  if (rc == VSG_OK)
    rc = pose_chain_enqueue(F, c, S, A.edge_feat, A.edge_slot, (const int32_t *)A.status, Tcw, cam, inv_level_sigma2,
                            nlevels, hold_round, T.pin_extra + L.pPose);
  const bool walked = launched == VSG_OK;
  const hipError_t e = hipStreamSynchronize(c->stream);  // an error after an enqueue waits for the stream too
  if (e != hipSuccess || !walked) return VSG_ERR_HIP;
  // the walk kernel ran to its end: what the window kernel's waves took from the counter is known and is accounted for,
  // whatever else went wrong, so that the thread's next call starts from the right base
  *st = *(const walkdev::Status *)(hp + L.pStatus);
  const int acc = T.wc.account(st->overflow_sum);
  if (rc != VSG_OK) return VSG_ERR_HIP;
  if (acc != VSG_OK) return acc;
  return (st->flags & walkdev::kStOverflow) ? VSG_ERR_HIP : VSG_OK;  // a list outside the array: never seen
}

bool octaves_in_pyramid(const vsg_frame *F, int nlevels) {
  const size_t n = (size_t)F->n < F->h_kps.size() ? (size_t)F->n : F->h_kps.size();
  for (size_t i = 0; i < n; i++)
    if (F->h_kps[i].octave < 0 || F->h_kps[i].octave >= nlevels) return false;
  return true;
}

const int kAngleStride = (int)sizeof(KeyPointPOD);

static_assert(sizeof(walkdev::Status) == VSG_WALK_ST_WORDS * 4, "vsg_debug_track_walk hands the status back as int32 words");

}  // namespace

extern "C" {

// Test hook (include/vsg_orb_debug.h): k_track_walk alone on the caller's lists.
int vsg_debug_track_walk(int form, int nq, int nf, int n_ent, const uint32_t *ent, const int32_t *off, const int32_t *cnt,
                         int cap, const uint8_t *q_valid, const uint8_t *observed, const uint8_t *blocked_in,
                         const float *q_angle, const float *t_angle, const int32_t *q_slot, const int32_t *slots_in,
                         const uint8_t *slot_observed, int n_slots, int check_orientation, int min_matches, float nnratio,
                         int32_t *train_match, uint8_t *train_blocked, int32_t *feat_slots, uint8_t *feat_observed,
                         int32_t *edge_feat, int32_t *edge_slot, int32_t *status) {
  if (!ent || !off || !cnt || !q_angle || !t_angle || !train_match || !train_blocked || !feat_slots || !feat_observed ||
      !edge_feat || !edge_slot || !status)
    return VSG_ERR_INVALID;
  if (form != walkdev::kFormLast && form != walkdev::kFormLocal) return VSG_ERR_INVALID;
  if (nq < 0 || nf < 0 || n_ent < 0 || cap < 0 || n_slots < 0 || nf > 32768) return VSG_ERR_INVALID;
  if (slot_observed) {
    for (int q = 0; q_slot && q < nq; q++)
      if (q_slot[q] < -1 || q_slot[q] >= n_slots) return VSG_ERR_INVALID;
    for (int i = 0; slots_in && i < nf; i++)
      if (slots_in[i] < -1 || slots_in[i] >= n_slots) return VSG_ERR_INVALID;
  }
  if (walk_over_cap(nq, nf)) return VSG_ERR_CAPACITY;
  // everything the kernel indexes has been bounded (the lists: list_ok, in the kernel); nothing has been enqueued
  int device = 0, rc = VSG_OK;
  if (hipGetDevice(&device) != hipSuccess) return VSG_ERR_NO_DEVICE;
  ThreadCtx *c = thread_ctx(device, &rc);
  if (!c) return rc;
  const size_t Q = (size_t)nq, N = (size_t)nf;
  // one block with the same layout in the pinned and in the device arena: the inputs, then what the kernel writes to
  // device memory (the edge list and the status, as in the chain calls); behind it, pinned only, what it writes for the host
  Stage s;
  const size_t oEnt = s.add((size_t)n_ent * 4), oOff = s.add(Q * 4), oCnt = s.add(Q * 4), oValid = s.add(Q), oObs = s.add(Q),
               oBlk = s.add(N), oQa = s.add(Q * 4), oTa = s.add(N * 4), oQs = s.add(Q * 4), oSi = s.add(N * 4),
               oSo = s.add((size_t)n_slots);
  const size_t oFeat = s.add(N * 4), oSlot = s.add(N * 4), oStatus = s.add(sizeof(walkdev::Status));
  const size_t dev_total = s.total;
  const size_t pTm = s.add(N * 4), pTb = s.add(N), pFs = s.add(N * 4), pFo = s.add(N);
  const size_t pStatus = s.add(sizeof(walkdev::Status));
  rc = ctx_reserve(c, s.total, dev_total);
  if (rc != VSG_OK) return rc;
  uint8_t *hp = c->h_pin, *dp = c->d_pin, *dv = c->d_buf;
  auto put = [&](size_t at, const void *src, size_t bytes) {
    if (src && bytes) memcpy(hp + at, src, bytes);
  };
  put(oEnt, ent, (size_t)n_ent * 4), put(oOff, off, Q * 4), put(oCnt, cnt, Q * 4), put(oValid, q_valid, Q);
  put(oObs, observed, Q), put(oBlk, blocked_in, N), put(oQa, q_angle, Q * 4), put(oTa, t_angle, N * 4);
  put(oQs, q_slot, Q * 4), put(oSi, slots_in, N * 4), put(oSo, slot_observed, (size_t)n_slots);
  // the outputs start as the caller's arrays are, so that an entry the kernel leaves out shows as what the caller put there
  put(oFeat, edge_feat, N * 4), put(oSlot, edge_slot, N * 4), put(pTm, train_match, N * 4), put(pTb, train_blocked, N);
  put(pFs, feat_slots, N * 4), put(pFo, feat_observed, N);
  memset(hp + oStatus, 0, sizeof(walkdev::Status)), memset(hp + pStatus, 0, sizeof(walkdev::Status));
  walkdev::Args A;
  memset(&A, 0, sizeof(A));
  A.form = form, A.nq = nq, A.nf = nf;
  A.inline_len = kWinInline, A.cap = cap, A.list_total = n_ent;
  A.check_orientation = check_orientation != 0, A.min_matches = min_matches, A.nnratio = nnratio;
  A.ent = (const uint32_t *)(dv + oEnt), A.off = (const int32_t *)(dv + oOff), A.cnt = (const int32_t *)(dv + oCnt);
  A.q_valid = q_valid ? dv + oValid : nullptr, A.observed = observed ? dv + oObs : nullptr;
  A.blocked_in = blocked_in ? dv + oBlk : nullptr;
  A.q_angle = dv + oQa, A.t_angle = dv + oTa, A.q_angle_stride = A.t_angle_stride = 4;
  A.q_slot = q_slot ? (const int32_t *)(dv + oQs) : nullptr, A.slots_in = slots_in ? (const int32_t *)(dv + oSi) : nullptr;
  A.slot_observed = slot_observed ? dv + oSo : nullptr;
  A.train_match = (int32_t *)(dp + pTm), A.train_blocked = dp + pTb, A.feat_slots = (int32_t *)(dp + pFs);
  A.feat_observed = dp + pFo;
  A.edge_feat = (int32_t *)(dv + oFeat), A.edge_slot = (int32_t *)(dv + oSlot);
  A.status = (walkdev::Status *)(dv + oStatus), A.status2 = (walkdev::Status *)(dp + pStatus);
  hipStream_t st = c->stream;
  TRY_HIP(hipMemcpyAsync(dv, hp, dev_total, hipMemcpyHostToDevice, st));
  bool failed = walk_launch(st, A) != VSG_OK;
  if (!failed && hipMemcpyAsync(hp + oFeat, dv + oFeat, dev_total - oFeat, hipMemcpyDeviceToHost, st) != hipSuccess)
    failed = true;
  if (hipStreamSynchronize(st) != hipSuccess || failed) return VSG_ERR_HIP;
  // the kernel writes its status twice, to device memory for the pose solve and to the pinned arena for the host
  if (memcmp(hp + oStatus, hp + pStatus, sizeof(walkdev::Status)) != 0) return VSG_ERR_HIP;
  memcpy(status, hp + pStatus, sizeof(walkdev::Status));
  if (((const walkdev::Status *)(hp + pStatus))->flags & walkdev::kStOverflow) return VSG_OK;  // nothing else was written
  if (nf > 0) {
    memcpy(train_match, hp + pTm, N * 4), memcpy(train_blocked, hp + pTb, N), memcpy(feat_slots, hp + pFs, N * 4);
    memcpy(feat_observed, hp + pFo, N), memcpy(edge_feat, hp + oFeat, N * 4), memcpy(edge_slot, hp + oSlot, N * 4);
  }
  return VSG_OK;
}

int vsg_frame_track_with_motion_model(vsg_frame *cur, vsg_frame *last, vsg_mappoints *mp, const int32_t *last_slots,
                                      const vsg_frame_pose *cur_pose, const vsg_frame_pose *last_pose, float mb, int mono,
                                      float th, const float *scale_factors, int nlevels, int check_orientation,
                                      const vsg_pose_se3 *Tcw, const float *inv_level_sigma2, int hold_round,
                                      int32_t *feat_slots_out, int32_t *train_match, uint8_t *outlier, float *chi2,
                                      vsg_track_result *res) {
  if (!Tcw || !inv_level_sigma2 || !res || !outlier || !feat_slots_out) return VSG_ERR_INVALID;
  if (hold_round != -1 && hold_round != 2) return VSG_ERR_INVALID;
  int dir = 0;
  int rc = track_last_check(cur, last, mp, last_slots, cur_pose, last_pose, mb, mono, scale_factors, nlevels, &dir);
  if (rc != VSG_OK) return rc;
  StoreView S;
  if (!store_view(mp, &S) || !octaves_in_pyramid(cur, nlevels)) return VSG_ERR_INVALID;
  // everything the kernels index has been bounded; nothing has been enqueued
  const int nf = cur->n, nq = last->n;
  if (nf > 0 && nq > 0 && walk_over_cap(nq, nf)) return VSG_ERR_CAPACITY;
  // an error from here on leaves *res, the outputs and a pending hold as they were: R becomes *res on success only
  vsg_track_result R;
  memset(&R, 0, sizeof(R));
  R.direction = dir;
  pose_result_input(Tcw, 0, &R.pose);
  if (nf == 0 || nq == 0) {  // both searches find nothing (:2958, :2967)
    for (int i = 0; i < nf; i++) {
      feat_slots_out[i] = -1;
      if (train_match) train_match[i] = -1;
    }
    R.wide = 1;
    *res = R;
    return 0;
  }
  const TrackLayout L(nf);
  walkdev::Status st;
  TrackSearch T;
  for (int pass = 0; pass < 2; pass++) {
    const float th_now = pass ? 2 * th : th;  // :2961: every feature is free again, the window twice as wide
    rc = with_retry([&]() -> int {
      T = TrackSearch();
      int r = track_last_enqueue(&T, cur, last, mp, last_slots, cur_pose, th_now, dir, scale_factors, nlevels, L.pin_total,
                                 L.dev_total);
      if (r != VSG_OK) return r;
      walkdev::Args A;
      memset(&A, 0, sizeof(A));
      A.form = walkdev::kFormLast, A.nq = nq, A.nf = nf;
      A.check_orientation = check_orientation != 0, A.min_matches = 20;
      A.observed = T.d_observed;
      A.q_angle = &last->d_kps->angle, A.t_angle = &cur->d_kps->angle, A.q_angle_stride = A.t_angle_stride = kAngleStride;
      A.q_slot = T.d_slots, A.slot_observed = store_observed_dev(mp);
      return walk_solve_wait(T, L, A, cur, S, Tcw, cur_pose, inv_level_sigma2, nlevels, hold_round, &st);
    });
    if (rc != VSG_OK) return rc;
    if (pass == 0) R.n_search = st.nmatches;
    if (st.nmatches >= 20) break;
    R.wide = 1;
  }
  const uint8_t *hp = T.c->h_pin + T.pin_extra;
  const int32_t *tm = (const int32_t *)(hp + L.pTm), *fs = (const int32_t *)(hp + L.pFs);
  const uint8_t *fo = hp + L.pFo;
  R.n_matches_searched = st.nmatches, R.n_matches = st.nmatches;
  std::vector<int32_t> feat;  // the edge list read back: the features with a slot, ascending
  for (int i = 0; i < nf; i++)
    if (fs[i] >= 0) feat.push_back(i);
  const bool solved = st.nmatches >= 20 && !(st.flags & walkdev::kStFewEdges);
  if (solved && (int)feat.size() != st.n_edges) return VSG_ERR_HIP;
  memcpy(feat_slots_out, fs, (size_t)nf * 4);
  if (train_match) memcpy(train_match, tm, (size_t)nf * 4);
  if (st.nmatches < 20) {  // :2967: the pose stays, nothing is flagged
    *res = R;
    return st.nmatches;
  }
  R.optimized = 1;
  if (!solved) {  // Optimizer.cc:1251
    for (int i = 0; i < nf; i++)
      if (fs[i] >= 0) outlier[i] = 0;
    pose_result_input(Tcw, st.n_edges, &R.pose);
  } else {
    pose_chain_finish(cur, T.c, T.pin_extra + L.pPose, feat.data(), st.n_edges, outlier, chi2, &R.pose);
    if (R.pose.held) {  // the caller runs the plane step, _resume and the discard
      *res = R;
      return st.nmatches;
    }
  }
  int n_matches = st.nmatches, n_map = 0;  // :2980-3005
  for (int i = 0; i < nf; i++) {
    if (feat_slots_out[i] < 0) continue;
    if (outlier[i])
      feat_slots_out[i] = -1, outlier[i] = 0, n_matches--;
    else if (fo[i])
      n_map++;
  }
  R.n_matches = n_matches, R.n_matches_map = n_map;
  *res = R;
  return n_matches;
}

int vsg_frame_track_local_map(vsg_frame *F, vsg_mappoints *mp, int n, const int32_t *slots, const uint8_t *skip,
                              const vsg_frame_pose *pose, float viewing_cos_limit, float th, float nnratio, int far_points,
                              float th_far_points, const float *scale_factors, int nlevels, const int32_t *feat_slots_in,
                              const vsg_pose_se3 *Tcw, const float *inv_level_sigma2, int hold_round, int only_tracking,
                              int drop_outliers, int32_t *feat_slots_out, int32_t *train_match, uint8_t *outlier,
                              float *chi2, uint8_t *in_view, float *proj_x, float *proj_y, vsg_track_local_result *res) {
  if (!Tcw || !inv_level_sigma2 || !res || !outlier || !feat_slots_out || !feat_slots_in) return VSG_ERR_INVALID;
  if (hold_round != -1 && hold_round != 2) return VSG_ERR_INVALID;
  if (nlevels < 1 || nlevels > 16) return VSG_ERR_INVALID;
  int rc = track_local_check(F, mp, n, slots, pose, scale_factors, nlevels);
  if (rc != VSG_OK) return rc;
  StoreView S;
  if (!store_view(mp, &S) || !octaves_in_pyramid(F, nlevels)) return VSG_ERR_INVALID;
  const int nf = F->n, nq = n;
  for (int i = 0; i < nf; i++)
    if (feat_slots_in[i] >= S.capacity) return VSG_ERR_INVALID;
  // everything the kernels index has been bounded; nothing has been enqueued
  if (nf > 0 && walk_over_cap(nq, nf)) return VSG_ERR_CAPACITY;
  // an error from here on leaves *res, the outputs and a pending hold as they were: R becomes *res on success only
  vsg_track_local_result R;
  memset(&R, 0, sizeof(R));
  pose_result_input(Tcw, 0, &R.pose);
  if (nf == 0) {  // no feature to match or to solve with: nothing is enqueued, the per-query outs stay as they are
    *res = R;
    return 0;
  }
  std::vector<int32_t> own_slots;  // slots == NULL is slot i: the walk reads the queries' slots from the staged list
  if (!slots && nq > 0) {
    own_slots.resize((size_t)nq);
    for (int i = 0; i < nq; i++) own_slots[(size_t)i] = i;
    slots = own_slots.data();
  }
  const TrackLayout L(nf, true);
  walkdev::Status st;
  TrackSearch T;
  rc = with_retry([&]() -> int {
    T = TrackSearch();
    int r = track_local_enqueue(&T, F, mp, nq, slots, skip, pose, viewing_cos_limit, th, far_points, th_far_points,
                                scale_factors, nlevels, L.pin_total, L.dev_total);
    if (r != VSG_OK) return r;
    memcpy(T.c->h_pin + T.pin_extra + L.pSlotsIn, feat_slots_in, (size_t)nf * 4);
    walkdev::Args A;
    memset(&A, 0, sizeof(A));
    A.form = walkdev::kFormLocal, A.nq = nq, A.nf = nf;
    A.check_orientation = 0, A.min_matches = 0, A.nnratio = nnratio;  // no rotation filter; the solve always runs
    A.q_valid = T.d_valid, A.observed = T.d_observed;
    A.q_slot = T.d_slots, A.slot_observed = store_observed_dev(mp);
    // blocked on entry = the entry slot's point is observed: k_track_walk derives it from these two
    A.slots_in = (const int32_t *)(T.c->d_pin + T.pin_extra + L.pSlotsIn);
    return walk_solve_wait(T, L, A, F, S, Tcw, pose, inv_level_sigma2, nlevels, hold_round, &st);
  });
  if (rc != VSG_OK) return rc;
  const uint8_t *hp = T.c->h_pin + T.pin_extra;
  const int32_t *tm = (const int32_t *)(hp + L.pTm), *fs = (const int32_t *)(hp + L.pFs);
  const uint8_t *fo = hp + L.pFo;
  std::vector<int32_t> feat;  // the edge list read back: the features with a slot, ascending
  for (int i = 0; i < nf; i++)
    if (fs[i] >= 0) feat.push_back(i);
  const bool solved = !(st.flags & walkdev::kStFewEdges);
  if ((int)feat.size() != st.n_edges) return VSG_ERR_HIP;
  int to_match = 0;  // nToMatch (Tracking.cc:3460)
  for (int q = 0; q < nq; q++) to_match += T.h_valid[q];
  R.n_to_match = to_match, R.n_matches_searched = st.nmatches, R.walk_rounds = st.rounds;
  memcpy(feat_slots_out, fs, (size_t)nf * 4);
  if (train_match) memcpy(train_match, tm, (size_t)nf * 4);
  if (in_view && nq > 0) memcpy(in_view, T.h_valid, (size_t)nq);
  if (proj_x && nq > 0) memcpy(proj_x, T.h_x, (size_t)nq * 4);
  if (proj_y && nq > 0) memcpy(proj_y, T.h_y, (size_t)nq * 4);
  if (!solved) {  // Optimizer.cc:1251
    for (int i = 0; i < nf; i++)
      if (fs[i] >= 0) outlier[i] = 0;
    pose_result_input(Tcw, st.n_edges, &R.pose);
  } else {
    pose_chain_finish(F, T.c, T.pin_extra + L.pPose, feat.data(), st.n_edges, outlier, chi2, &R.pose);
    if (R.pose.held) {  // the caller runs the plane step, _resume, the statistics and the drop
      *res = R;
      return 0;
    }
  }
  R.n_matches_inliers = track_local_stats(nf, feat_slots_out, outlier, fo, only_tracking, drop_outliers);  // :3074-3095
  *res = R;
  return R.n_matches_inliers;
}

}  // extern "C"
