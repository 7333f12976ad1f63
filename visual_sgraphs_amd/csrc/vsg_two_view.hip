// vsg_two_view.hip -- TwoViewReconstruction::Reconstruct on two resident frames or on keypoints the caller holds
// (TwoViewReconstruction.cc; Tracking.cc:2568): vsg_frame_two_view_reconstruct, vsg_two_view_reconstruct, and the host-only
// draw of the minimal sets, vsg_two_view_draw_sets.  The arithmetic is vsg_two_view.h.
//
// The host compacts the matches while it range-checks them (it has to walk them anyway) and takes Normalize's four sums
// per frame from the frames' host mirrors, in index order; then four kernels back to back on the calling thread's stream
// and one wait:
//   k_tv_prepare      one lane per match: the two keypoints out of the resident frames (or the staged coordinates of the
//                     host-array form) and their normalised coordinates into the calling thread's device arena;
//   k_tv_hypotheses   one WAVE per (iteration, model), 2 * n_iter workgroups of one wave.  The 16 x 9 / 8 x 9 system
//                     lives in LDS (25 x 9 doubles: it does not fit the register file, and scratch is what LDS is for):
//                     every lane takes the column sums, on identical bits, and lane r rotates row r (vsg_jacobi.h).  The
//                     rest of the solve runs on every lane, uniform.  The 64 lanes stride over the matches with a
//                     wave-uniform trip count; the two score terms of the 64 matches of a trip are added IN ORDER, lane
//                     by lane, by every lane (v_readlane feeds a uniform add): 2 * N dependent float additions per wave;
//                     the score and the 18 (H21 | H12) or 9 (F21) floats of the model go to the arena, no inlier matrix;
//   k_tv_select       one wave: both first maxima, the two winners' matrices out of the arena (solving them again would
//                     cost two more Jacobis in a row, more than everything else in the call), their inlier flags, RH, the
//                     model, its 3 x 3 decomposition and the 4 or 8 (R, t);
//   k_tv_check_rt     one wave per motion hypothesis: CheckRT's verdict per inlier match, nGood by popcount of the
//                     ballot, the cosine of rank min(50, nGood - 1) by a rank count through LDS tiles.
// The choice among the motion hypotheses, acos and the parallax gate run on the host behind the wait (two_view::finish),
// which also scatters the chosen hypothesis's points to the caller's arrays.
// No atomics, no grid-wide barrier, nothing spins; every loop is bounded by an argument or by a compile-time sweep count;
// every index a kernel follows was range-checked on the host.  All stores are plain vector stores.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "vsg_frame_int.h"
#include "vsg_two_view.h"

using namespace vsg;

namespace {

enum { kTvWaves = 1, kTvThreads = 64 * kTvWaves, kTvTile = 1024 };

struct TvArgs {
  const KeyPointPOD *kps1, *kps2;  // the resident frames' mvKeysUn, or nullptr:
  const float *raw;                // {u1, v1, u2, v2} per match, staged by the host-array form
  const int *pairs;                // [2 * N] {first, second}
  const int *sets;                 // [8 * n_iter]
  two_view::Norm nm1, nm2;
  float T1[9], T2inv[9], T2t[9], K[9];
  float sigma, inv_sigma2, rh_threshold;
  int N, n_iter;
  // device arena
  two_view::Match *m;              // [N]
  float *score;                    // [2 * n_iter]: H then F
  float *models;                   // [18 * 2 * n_iter]: H21 | H12 of every H hypothesis, then F21 | nine unused of every F one
  uint8_t *in_h, *in_f;            // [N]
  two_view::Selected *sel;
  uint8_t *state;                  // [8 * N]
  float *cosv;                     // [8 * N]
  // pinned outputs
  two_view::Selected *sel_out;
  int *n_good;                     // [8]
  float *cosk;                     // [8]
  uint8_t *state_out;              // [8 * N]
  float *pos_out;                  // [24 * N]
  uint8_t *in_h_out, *in_f_out;    // [N] or nullptr
  float *score_out;                // [2 * n_iter] or nullptr
};

// the Jacobi's matrix in LDS: every lane reads it, lane r rotates row r, a barrier of the one-wave workgroup in between
template <int M, int N>
struct JacobiLds {
  static constexpr bool kUnrolled = false;
  double *w;
  int lane;
  __device__ __forceinline__ double &at(int r, int c) { return w[r * N + c]; }
  template <class F>
  __device__ __forceinline__ void rows(F f) {
    if (lane < M + N) f(lane);
  }
  __device__ __forceinline__ void sync() { __syncthreads(); }
};

__global__ __launch_bounds__(256) void k_tv_prepare(TvArgs a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.N) return;
  float u1, v1, u2, v2;
  if (a.kps1) {
    const int i1 = a.pairs[2 * i], i2 = a.pairs[2 * i + 1];  // inside their frames: the host checked
    u1 = a.kps1[i1].x, v1 = a.kps1[i1].y, u2 = a.kps2[i2].x, v2 = a.kps2[i2].y;
  } else {
    u1 = a.raw[4 * (size_t)i], v1 = a.raw[4 * (size_t)i + 1], u2 = a.raw[4 * (size_t)i + 2], v2 = a.raw[4 * (size_t)i + 3];
  }
  a.m[i] = two_view::make_match(a.nm1, a.nm2, u1, v1, u2, v2);
}

// hypothesis `it` of a model on the one-wave workgroup; w = 25 x 9 doubles of LDS
__device__ __forceinline__ void solve_h(const TvArgs &a, int it, double *w, int lane, float *H21, float *H12) {
  const int *set = a.sets + 8 * (size_t)it;  // entries inside [0, N): the host checked
  JacobiLds<16, 9> s = {w, lane};
  two_view::hypothesis_h(
      s, [&](int j, float *p) { const two_view::Match &q = a.m[set[j]]; p[0] = q.x1, p[1] = q.y1, p[2] = q.x2, p[3] = q.y2; },
      a.T1, a.T2inv, H21, H12);
}
__device__ __forceinline__ void solve_f(const TvArgs &a, int it, double *w, int lane, float *F21) {
  const int *set = a.sets + 8 * (size_t)it;
  JacobiLds<8, 9> s = {w, lane};
  two_view::hypothesis_f(
      s, [&](int j, float *p) { const two_view::Match &q = a.m[set[j]]; p[0] = q.x1, p[1] = q.y1, p[2] = q.x2, p[3] = q.y2; },
      a.T1, a.T2t, F21);
}

// score + t1 of lane 0 + t2 of lane 0 + t1 of lane 1 + ... in that order, on every lane
__device__ __forceinline__ float ordered_add(float score, float t1, float t2) {
#pragma unroll
  for (int j = 0; j < 64; j++) {
    score = fadd(score, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t1), j)));
    score = fadd(score, __int_as_float(__builtin_amdgcn_readlane(__float_as_int(t2), j)));
  }
  return score;
}

__global__ __launch_bounds__(kTvThreads) void k_tv_hypotheses(TvArgs a) {
  __shared__ double s_w[25 * 9];
  const int lane = threadIdx.x, wv = blockIdx.x;  // wv < 2 * n_iter: the grid
  const bool is_f = wv >= a.n_iter;
  const int it = is_f ? wv - a.n_iter : wv;
  float H21[9], H12[9], F21[9];
  if (is_f)  // workgroup-uniform
    solve_f(a, it, s_w, lane, F21);
  else
    solve_h(a, it, s_w, lane, H21, H12);
  float score = 0.0f;
  for (int base = 0; base < a.N; base += 64) {  // wave-uniform trip count: every lane reaches the readlanes
    const int i = base + lane;
    float t1 = 0.0f, t2 = 0.0f;  // a lane past the last match adds +0: the sum keeps its bits
    if (i < a.N) {
      const two_view::Match q = a.m[i];
      if (is_f)
        two_view::score_f(F21, q, a.inv_sigma2, &t1, &t2);
      else
        two_view::score_h(H21, H12, q, a.inv_sigma2, &t1, &t2);
    }
    score = ordered_add(score, t1, t2);
  }
  if (lane == 0) {
    a.score[wv] = score;
    if (a.score_out) a.score_out[wv] = two_view::canonf(score);
    float *mo = a.models + 18 * (size_t)wv;
#pragma unroll
    for (int k = 0; k < 9; k++) mo[k] = is_f ? F21[k] : H21[k], mo[9 + k] = is_f ? 0.0f : H12[k];
  }
}

__global__ __launch_bounds__(kTvThreads) void k_tv_select(TvArgs a) {
  __shared__ float s_score[2 * two_view::kMaxIterations];
  const int lane = threadIdx.x;
  for (int k = lane; k < 2 * a.n_iter; k += kTvThreads) s_score[k] = a.score[k];
  __syncthreads();
  // uniform: every lane walks the scores as the two loops do
  const int best_h = two_view::first_maximum(s_score, a.n_iter), best_f = two_view::first_maximum(s_score + a.n_iter, a.n_iter);
  float H21[9], H12[9], F21[9];
#pragma unroll
  for (int k = 0; k < 9; k++) H21[k] = H12[k] = F21[k] = 0.0f;
  if (best_h >= 0) {  // uniform loads
    const float *mo = a.models + 18 * (size_t)best_h;
#pragma unroll
    for (int k = 0; k < 9; k++) H21[k] = mo[k], H12[k] = mo[9 + k];
  }
  if (best_f >= 0) {
    const float *mo = a.models + 18 * (size_t)(a.n_iter + best_f);
#pragma unroll
    for (int k = 0; k < 9; k++) F21[k] = mo[k];
  }
  int n_in_h = 0, n_in_f = 0;
  for (int base = 0; base < a.N; base += 64) {
    const int i = base + lane;
    bool ih = false, jf = false;
    if (i < a.N) {
      const two_view::Match q = a.m[i];
      float t1, t2;
      ih = best_h >= 0 && two_view::score_h(H21, H12, q, a.inv_sigma2, &t1, &t2);
      jf = best_f >= 0 && two_view::score_f(F21, q, a.inv_sigma2, &t1, &t2);
      a.in_h[i] = ih ? 1 : 0, a.in_f[i] = jf ? 1 : 0;
      if (a.in_h_out) a.in_h_out[i] = ih ? 1 : 0;
      if (a.in_f_out) a.in_f_out[i] = jf ? 1 : 0;
    }
    n_in_h += __popcll(__ballot(ih)), n_in_f += __popcll(__ballot(jf));
  }
  two_view::Selected S;
  two_view::fill_selected(S, best_h, best_f, best_h >= 0 ? s_score[best_h] : 0.0f, best_f >= 0 ? s_score[a.n_iter + best_f] : 0.0f,
                          H21, F21, n_in_h, n_in_f, a.K, a.rh_threshold);
  if (lane == 0) *a.sel = S, *a.sel_out = S;
}

__global__ __launch_bounds__(kTvThreads) void k_tv_check_rt(TvArgs a) {
  __shared__ float s_cos[kTvTile];
  const int lane = threadIdx.x, h = blockIdx.x;  // h < 8: the grid
  const int n_motion = a.sel->n_motion, model = a.sel->model;
  if (h >= n_motion) {  // workgroup-uniform
    if (lane == 0) a.n_good[h] = 0, a.cosk[h] = 0.0f;
    return;
  }
  const two_view::Motion mo = a.sel->motion[h];
  const two_view::RtSetup c = two_view::rt_setup(mo, a.K, a.sigma);
  const uint8_t *in = model == two_view::kModelH ? a.in_h : a.in_f;
  uint8_t *state = a.state + (size_t)h * a.N, *state_out = a.state_out + (size_t)h * a.N;
  float *cosv = a.cosv + (size_t)h * a.N, *pos_out = a.pos_out + 3 * (size_t)h * a.N;
  int n_good = 0;
  for (int base = 0; base < a.N; base += 64) {
    const int i = base + lane;
    int st = two_view::kRtSkipped;
    if (i < a.N) {
      float p[3] = {0.0f, 0.0f, 0.0f}, cs = 0.0f;
      if (in[i]) st = two_view::check_rt_match(c, a.m[i], p, &cs);  // :820
      state[i] = (uint8_t)st, state_out[i] = (uint8_t)st, cosv[i] = cs;
      pos_out[3 * (size_t)i] = p[0], pos_out[3 * (size_t)i + 1] = p[1], pos_out[3 * (size_t)i + 2] = p[2];
    }
    n_good += __popcll(__ballot(st != two_view::kRtSkipped));
  }
  __syncthreads();  // state and cosv are read back below, by other lanes than wrote them
  // two_view::ranked_cosine: candidate j = base + lane, the counted values in tiles through LDS (NaN = not counted: no
  // comparison with it holds); the first candidate (ascending j) that holds rank idx
  const int idx = 50 < n_good - 1 ? 50 : n_good - 1;
  float found = __builtin_nanf("");
  bool done = n_good <= 0;
  for (int base = 0; base < a.N && !done; base += 64) {  // `done` is workgroup-uniform
    const int j = base + lane;
    const bool cand = j < a.N && state[j] != two_view::kRtSkipped;
    const float cj = cand ? cosv[j] : 0.0f;
    int lo = 0, le = 0;
    for (int t0 = 0; t0 < a.N; t0 += kTvTile) {
      const int tn = a.N - t0 < kTvTile ? a.N - t0 : kTvTile;
      __syncthreads();
      for (int t = lane; t < tn; t += 64) s_cos[t] = state[t0 + t] != two_view::kRtSkipped ? cosv[t0 + t] : __builtin_nanf("");
      __syncthreads();
      for (int t = 0; t < tn; t++) {
        const float v = s_cos[t];
        lo += v < cj ? 1 : 0, le += v <= cj ? 1 : 0;
      }
    }
    const unsigned long long hit = __ballot(cand && lo <= idx && idx < le);
    if (hit) {
      found = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(cj), __builtin_ctzll(hit)));
      done = true;
    }
  }
  if (lane == 0) a.n_good[h] = n_good, a.cosk[h] = two_view::canonf(found);
}

// what both exported forms share behind their own checks.  kps1 / kps2: the resident frames' keypoints (device), or
// nullptr with xy1 / xy2 (host) to stage the matched coordinates from.  nm1 / nm2: Normalize's numbers of the two frames.
int tv_run(int device, const KeyPointPOD *kps1, const KeyPointPOD *kps2, const float *xy1, const float *xy2, int n1,
           const two_view::Norm &nm1, const two_view::Norm &nm2, int N, const int32_t *pairs, const float *K,
           const vsg_two_view_params &P, int n_iter, const int32_t *sets, vsg_two_view_result *res, uint8_t *triangulated,
           float *x3d, uint8_t *inlier_h, uint8_t *inlier_f, float *score_h, float *score_f) {
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(device, &rc);
  if (!c) return rc;
  const size_t n = (size_t)N, H = (size_t)n_iter;
  Stage st, dv;
  const size_t oPairs = st.add(n * 8), oSets = st.add(H * 32), oRaw = st.add(kps1 ? 0 : n * 16);
  const size_t oSel = st.add(sizeof(two_view::Selected)), oGood = st.add(8 * 4), oCos = st.add(8 * 4);
  const size_t oState = st.add(8 * n), oPos = st.add(96 * n);
  const size_t oInH = st.add(inlier_h ? n : 0), oInF = st.add(inlier_f ? n : 0);
  const bool want_scores = score_h || score_f;
  const size_t oScore = st.add(want_scores ? H * 8 : 0);
  const size_t dM = dv.add(n * sizeof(two_view::Match)), dScore = dv.add(H * 8), dModels = dv.add(H * 144), dInH = dv.add(n), dInF = dv.add(n);
  const size_t dSel = dv.add(sizeof(two_view::Selected)), dState = dv.add(8 * n), dCos = dv.add(32 * n);
  rc = ctx_reserve(c, st.total, dv.total);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_pin, *b = c->d_buf;
  memcpy(h + oPairs, pairs, n * 8), memcpy(h + oSets, sets, H * 32);
  if (!kps1) {
    float *raw = (float *)(h + oRaw);
    for (int i = 0; i < N; i++) {
      const size_t p = (size_t)pairs[2 * i], q = (size_t)pairs[2 * i + 1];
      raw[4 * (size_t)i] = xy1[2 * p], raw[4 * (size_t)i + 1] = xy1[2 * p + 1];
      raw[4 * (size_t)i + 2] = xy2[2 * q], raw[4 * (size_t)i + 3] = xy2[2 * q + 1];
    }
  }
  TvArgs a;
  memset(&a, 0, sizeof a);
  a.kps1 = kps1, a.kps2 = kps2, a.raw = kps1 ? nullptr : (const float *)(d + oRaw);
  a.pairs = (const int *)(d + oPairs), a.sets = (const int *)(d + oSets);
  a.nm1 = nm1, a.nm2 = nm2;
  float T2[9];
  two_view::norm_matrix(nm1, a.T1), two_view::norm_matrix(nm2, T2);
  two_view::inverse3(T2, a.T2inv), two_view::transpose3(T2, a.T2t);
  memcpy(a.K, K, sizeof a.K);
  a.sigma = P.sigma, a.inv_sigma2 = two_view::inv_sigma_square(P.sigma), a.rh_threshold = P.rh_threshold;
  a.N = N, a.n_iter = n_iter;
  a.m = (two_view::Match *)(b + dM), a.score = (float *)(b + dScore), a.models = (float *)(b + dModels), a.in_h = b + dInH, a.in_f = b + dInF;
  a.sel = (two_view::Selected *)(b + dSel), a.state = b + dState, a.cosv = (float *)(b + dCos);
  a.sel_out = (two_view::Selected *)(d + oSel), a.n_good = (int *)(d + oGood), a.cosk = (float *)(d + oCos);
  a.state_out = d + oState, a.pos_out = (float *)(d + oPos);
  a.in_h_out = inlier_h ? d + oInH : nullptr, a.in_f_out = inlier_f ? d + oInF : nullptr;
  a.score_out = want_scores ? (float *)(d + oScore) : nullptr;
  hipLaunchKernelGGL(k_tv_prepare, dim3((N + 255) / 256), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_tv_hypotheses, dim3(2 * n_iter), dim3(kTvThreads), 0, c->stream, a);
  hipLaunchKernelGGL(k_tv_select, dim3(1), dim3(kTvThreads), 0, c->stream, a);
  hipLaunchKernelGGL(k_tv_check_rt, dim3(8), dim3(kTvThreads), 0, c->stream, a);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  const two_view::Selected S = *(const two_view::Selected *)(h + oSel);
  if (S.n_motion < 0 || S.n_motion > 8) return VSG_ERR_HIP;  // never: the kernel writes 0, 4 or 8
  const int *n_good = (const int *)(h + oGood);
  if (two_view::finish(S, n_good, (const float *)(h + oCos), P, res)) {
    const int k = two_view::chosen_motion(S, n_good, P.min_triangulated);
    two_view::scatter_outputs(n1, N, pairs, h + oState + (size_t)k * n, (const float *)(h + oPos) + 3 * (size_t)k * n,
                              S.model == two_view::kModelF, triangulated, x3d);
  }
  if (inlier_h) memcpy(inlier_h, h + oInH, n);
  if (inlier_f) memcpy(inlier_f, h + oInF, n);
  if (score_h) memcpy(score_h, h + oScore, H * 4);
  if (score_f) memcpy(score_f, h + oScore + H * 4, H * 4);
  return VSG_OK;
}

// what both forms refuse alike; *N = the number of matches, pairs filled
int tv_check(int n1, int n2, const int32_t *matches12, const float *K, const vsg_two_view_params *params, int n_iter,
             const int32_t *sets, const vsg_two_view_result *res, const uint8_t *triangulated, const float *x3d,
             std::vector<int32_t> *pairs, int *N) {
  if (!matches12 || !sets || !res || !triangulated || !x3d || n1 < 1 || n2 < 1) return VSG_ERR_INVALID;
  if (!two_view::params_ok(K, params, n_iter)) return VSG_ERR_INVALID;
  pairs->resize(2 * (size_t)n1);
  *N = two_view::compact_matches(n1, n2, matches12, pairs->data());
  if (*N < 8) return VSG_ERR_INVALID;  // an entry out of range (-1) included
  return two_view::sets_ok(*N, n_iter, sets) ? VSG_OK : VSG_ERR_INVALID;
}

}  // namespace

extern "C" {

void vsg_two_view_default_params(vsg_two_view_params *p) {
  if (!p) return;
  p->sigma = 1.0f, p->rh_threshold = 0.50f, p->min_parallax = 1.0f, p->min_triangulated = 50;
}

int vsg_frame_two_view_reconstruct(vsg_frame *f1, vsg_frame *f2, const int32_t *matches12, const float K[9],
                                   const vsg_two_view_params *params, int n_iter, const int32_t *sets,
                                   vsg_two_view_result *res, uint8_t *triangulated, float *x3d, uint8_t *inlier_h,
                                   uint8_t *inlier_f, float *score_h, float *score_f) {
  if (frame_check(f1) != VSG_OK || frame_check(f2) != VSG_OK || f1->device != f2->device) return VSG_ERR_INVALID;
  // Normalize reads every keypoint in index order: from the host mirrors, which every upload and extraction keeps
  if ((int)f1->h_kps.size() != f1->n || (int)f2->h_kps.size() != f2->n) return VSG_ERR_INVALID;
  std::vector<int32_t> pairs;
  int N = 0;
  const int rc = tv_check(f1->n, f2->n, matches12, K, params, n_iter, sets, res, triangulated, x3d, &pairs, &N);
  if (rc != VSG_OK) return rc;
  // ---- nothing is refused from here on
  const vsg_keypoint *k1 = f1->h_kps.data(), *k2 = f2->h_kps.data();
  const two_view::Norm nm1 = two_view::normalize(f1->n, [&](int i, float *x, float *y) { *x = k1[i].x, *y = k1[i].y; });
  const two_view::Norm nm2 = two_view::normalize(f2->n, [&](int i, float *x, float *y) { *x = k2[i].x, *y = k2[i].y; });
  return tv_run(f1->device, f1->d_kps, f2->d_kps, nullptr, nullptr, f1->n, nm1, nm2, N, pairs.data(), K, *params, n_iter, sets,
                res, triangulated, x3d, inlier_h, inlier_f, score_h, score_f);
}

int vsg_two_view_reconstruct(int device, const float *xy1, int n1, const float *xy2, int n2, const int32_t *matches12,
                             const float K[9], const vsg_two_view_params *params, int n_iter, const int32_t *sets,
                             vsg_two_view_result *res, uint8_t *triangulated, float *x3d, uint8_t *inlier_h,
                             uint8_t *inlier_f, float *score_h, float *score_f) {
  if (!xy1 || !xy2 || device < 0) return VSG_ERR_INVALID;
  std::vector<int32_t> pairs;
  int N = 0;
  const int rc = tv_check(n1, n2, matches12, K, params, n_iter, sets, res, triangulated, x3d, &pairs, &N);
  if (rc != VSG_OK) return rc;
  // ---- nothing is refused from here on
  const two_view::Norm nm1 = two_view::normalize(n1, [&](int i, float *x, float *y) { *x = xy1[2 * (size_t)i], *y = xy1[2 * (size_t)i + 1]; });
  const two_view::Norm nm2 = two_view::normalize(n2, [&](int i, float *x, float *y) { *x = xy2[2 * (size_t)i], *y = xy2[2 * (size_t)i + 1]; });
  return tv_run(device, nullptr, nullptr, xy1, xy2, n1, nm1, nm2, N, pairs.data(), K, *params, n_iter, sets, res, triangulated,
                x3d, inlier_h, inlier_f, score_h, score_f);
}

int vsg_two_view_draw_sets(int n, int n_iter, int (*random_int)(int lo, int hi, void *ctx), void *ctx, int32_t *sets) {
  if (n < 8 || n_iter < 0 || !sets) return VSG_ERR_INVALID;
  std::vector<int32_t> all((size_t)n), avail;
  for (int i = 0; i < n; i++) all[(size_t)i] = i;
  for (int it = 0; it < n_iter; it++) {
    avail = all;  // :84
    for (int j = 0; j < 8; j++) {
      const int hi = (int)avail.size() - 1;
      int randi;
      if (random_int) {
        randi = random_int(0, hi, ctx);
      } else {  // Random.cpp:47-50
        const int dd = hi - 0 + 1;
        randi = (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * dd) + 0;
      }
      if (randi < 0 || randi > hi) return VSG_ERR_INVALID;
      sets[8 * (size_t)it + j] = avail[(size_t)randi];
      avail[(size_t)randi] = avail.back();
      avail.pop_back();
    }
  }
  return VSG_OK;
}

}  // extern "C"
