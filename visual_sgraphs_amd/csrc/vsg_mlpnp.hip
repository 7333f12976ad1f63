// vsg_mlpnp.hip -- MLPnPsolver on a resident frame and resident map points (MLPnPsolver.cpp; Tracking.cc:3735, :3762):
// vsg_frame_mlpnp_ransac, and the two host-only pieces of the solver's set-up, vsg_mlpnp_ransac_parameters and
// vsg_mlpnp_draw_sets.  The arithmetic is vsg_mlpnp.h.
//
// The host compacts the features with a slot while it range-checks them (it has to walk them anyway); then three kernels
// back to back on the calling thread's stream, one wait:
//   k_mlpnp_points      one lane per correspondence: keypoint, octave and store position into the calling thread's device
//                       arena (mlpnp::make_point) -- the arena, so that two threads may solve on one store at the same time;
//   k_mlpnp_hypotheses  one WAVE per hypothesis, one wave per workgroup.  computePose runs on every lane on identical bits; the
//                       12 x 12 (planar 9 x 9) Jacobi work matrix lives in LDS, row r rotated by lane r, the workgroup's
//                       barrier between the pairs.  ONE wave per workgroup (kMlpnpWaves, asserted): the solve is a chain of
//                       dependent FP64 operations that leaves the other 63 lanes nothing to add, so a wave's cost is latency,
//                       LDS is 2.3 KB a wave and occupancy comes from the number of workgroups -- and the planar branch and the
//                       Jacobi's skipped pairs are per hypothesis, so a barrier shared by two waves would not be met by both.
//                       The 64 lanes then stride over the correspondences, the count is the popcount of the ballot;
//   k_mlpnp_select      one workgroup: the counts into LDS, mlpnp::select by every thread (uniform), the flags of the returned
//                       hypothesis scattered to the features, the result.
// Refine()'s solve over the best set (:305-337) is not run: the reference discards its result (vsg_mlpnp.h).
// No atomics, no grid-wide barrier, nothing spins; every loop is bounded by an argument or a compile-time constant; every
// index a kernel follows was range-checked on the host.  All stores are plain vector stores.
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "vsg_frame_int.h"
#include "vsg_mlpnp.h"

using namespace vsg;

namespace {

enum { kMlpnpWaves = 1, kMlpnpThreads = 64 * kMlpnpWaves };
// computePose synchronises with the workgroup's barrier at points that depend on the hypothesis: two waves cannot share it
static_assert(kMlpnpWaves == 1, "k_mlpnp_hypotheses runs one wave per workgroup");

struct MlpnpArgs {
  const KeyPointPOD *kps;  // the resident frame's mvKeysUn
  const float *pos;        // the store's GetWorldPos()
  const int *feat, *slot;  // [n]: the features with a slot, in feature order
  const int *sets;         // [6 * n_hyp]
  mlpnp::Camera cam;
  float sigma2[16], th2;
  int n_feat, n, n_hyp, min_inliers, max_its, first, n_iterations;
  // device arena
  mlpnp::Point *pts;       // [n]
  int *counts;             // [n_hyp]
  mlpnp::Pose *hyp;        // [n_hyp]
  // pinned outputs
  int *hyp_inliers;        // [n_hyp] or nullptr
  double *hyp_T;           // [12 * n_hyp] or nullptr
  uint8_t *inlier;         // [n_feat]
  vsg_mlpnp_result *res;
};

__global__ __launch_bounds__(256) void k_mlpnp_points(MlpnpArgs a) {
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= a.n) return;
  const KeyPointPOD kp = a.kps[a.feat[e]];  // inside the frame, octave inside [0, nlevels): the host checked
  const size_t s = (size_t)a.slot[e];       // inside the store: the host checked
  const float X[3] = {a.pos[3 * s], a.pos[3 * s + 1], a.pos[3 * s + 2]};
  const int o = kp.octave & 15;
  float sg = a.sigma2[0];
#pragma unroll
  for (int l = 1; l < 16; l++) sg = o == l ? a.sigma2[l] : sg;
  a.pts[e] = mlpnp::make_point(a.cam, kp.x, kp.y, sg, a.th2, X);
}

__global__ __launch_bounds__(kMlpnpThreads) void k_mlpnp_hypotheses(MlpnpArgs a) {
  __shared__ double s_w[kMlpnpWaves][mlpnp::kWork];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, k = blockIdx.x * kMlpnpWaves + wv;  // k < n_hyp: the grid
  int32_t set[6];  // read once: the sets lie in the pinned arena.  Entries inside [0, n): the host checked
#pragma unroll
  for (int j = 0; j < 6; j++) set[j] = a.sets[6 * (size_t)k + j];
  mlpnp::SerialTeam tm = {a.pts, set};
  mlpnp::Pose T;
  mlpnp::compute_pose(tm, s_w[wv], lane, 64, &T, nullptr);
  int count = 0;
  for (int base = 0; base < a.n; base += 64) {  // wave-uniform trip count: every lane reaches the ballot
    const int i = base + lane;
    const bool in = i < a.n && mlpnp::is_inlier(T, a.cam, a.pts[i < a.n ? i : 0]);
    count += __popcll(__ballot(in));
  }
  if (lane == 0) a.counts[k] = count, a.hyp[k] = T;
  if (a.hyp_T) {  // entry `lane` of [R | t] by selects: an index that varies by lane would put T into scratch
    double v = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++) v = lane == 4 * i + j ? T.R[3 * i + j] : v;
      v = lane == 4 * i + 3 ? T.t[i] : v;
    }
    if (lane < 12) a.hyp_T[12 * (size_t)k + lane] = mlpnp::canon(v);
  }
}

__global__ __launch_bounds__(256) void k_mlpnp_select(MlpnpArgs a) {
  __shared__ int s_counts[mlpnp::kMaxHypotheses];
  for (int k = threadIdx.x; k < a.n_hyp; k += 256) {
    const int c = a.counts[k];
    s_counts[k] = c;
    if (a.hyp_inliers) a.hyp_inliers[k] = c;
  }
  for (int i = threadIdx.x; i < a.n_feat; i += 256) a.inlier[i] = 0;
  __syncthreads();  // also orders the clearing above in front of the scatter below
  const mlpnp::Selection s = mlpnp::select(s_counts, a.first, a.n_iterations, a.max_its, a.min_inliers);  // uniform
  mlpnp::Pose T;
  int n_inliers = 0;
  if (s.pose >= 0) {  // uniform
    T = a.hyp[s.pose];
    n_inliers = s_counts[s.pose];
    for (int e = threadIdx.x; e < a.n; e += 256) a.inlier[a.feat[e]] = mlpnp::is_inlier(T, a.cam, a.pts[e]) ? 1 : 0;
  }
  if (threadIdx.x == 0) mlpnp::fill_result(s, s.pose >= 0 ? &T : nullptr, n_inliers, a.n, a.res);
}

}  // namespace

extern "C" {

int vsg_frame_mlpnp_ransac(vsg_frame *f, vsg_mappoints *mp, const int32_t *slots, float fx, float fy, float cx, float cy,
                           const float *level_sigma2, int nlevels, float th2, int min_inliers, int max_its, int first,
                           int n_iterations, int n_hyp, const int32_t *sets, uint8_t *inlier, vsg_mlpnp_result *res,
                           int32_t *hyp_inliers, double *hyp_T) {
  StoreView S;
  if (frame_check(f) != VSG_OK || !store_view(mp, &S)) return VSG_ERR_INVALID;
  if (f->nleft != -1) return VSG_ERR_UNSUPPORTED;  // KannalaBrandt8 pairs
  if (f->device != S.device || (int)f->h_kps.size() != f->n) return VSG_ERR_INVALID;
  int n = 0;
  if (!mlpnp::args_ok(f->n, slots, S.capacity, level_sigma2, nlevels, [&](int i) { return f->h_kps[(size_t)i].octave; }, th2,
                      min_inliers, max_its, first, n_iterations, n_hyp, sets, inlier, res, &n))
    return VSG_ERR_INVALID;
  // ---- nothing is refused from here on
  const int nf = f->n;
  if (n < min_inliers) {  // :111-115
    if (nf > 0) memset(inlier, 0, (size_t)nf);
    mlpnp::fill_no_more(n, res);
    return VSG_OK;
  }
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(f->device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n, H = (size_t)n_hyp, NF = (size_t)nf;
  Stage st, dv;
  const size_t oFeat = st.add(N * 4), oSlot = st.add(N * 4), oSets = st.add(H * 24), oIn = st.add(NF);
  const size_t oRes = st.add(sizeof(vsg_mlpnp_result)), oCnt = st.add(hyp_inliers ? H * 4 : 0), oT = st.add(hyp_T ? H * 96 : 0);
  const size_t dPts = dv.add(N * sizeof(mlpnp::Point)), dCnt = dv.add(H * 4), dHyp = dv.add(H * sizeof(mlpnp::Pose));
  rc = ctx_reserve(c, st.total, dv.total);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_pin, *b = c->d_buf;
  int32_t *hf = (int32_t *)(h + oFeat), *hs = (int32_t *)(h + oSlot);
  for (int i = 0, e = 0; i < nf; i++)
    if (slots[i] >= 0) hf[e] = i, hs[e] = slots[i], e++;
  memcpy(h + oSets, sets, H * 24);
  MlpnpArgs a;
  memset(&a, 0, sizeof a);
  a.kps = f->d_kps, a.pos = S.pos;
  a.feat = (const int *)(d + oFeat), a.slot = (const int *)(d + oSlot), a.sets = (const int *)(d + oSets);
  a.cam = mlpnp::Camera{fx, fy, cx, cy};
  for (int l = 0; l < 16; l++) a.sigma2[l] = level_sigma2[l < nlevels ? l : nlevels - 1];
  a.th2 = th2;
  a.n_feat = nf, a.n = n, a.n_hyp = n_hyp, a.min_inliers = min_inliers, a.max_its = max_its, a.first = first, a.n_iterations = n_iterations;
  a.pts = (mlpnp::Point *)(b + dPts), a.counts = (int *)(b + dCnt), a.hyp = (mlpnp::Pose *)(b + dHyp);
  a.hyp_inliers = hyp_inliers ? (int *)(d + oCnt) : nullptr, a.hyp_T = hyp_T ? (double *)(d + oT) : nullptr;
  a.inlier = d + oIn, a.res = (vsg_mlpnp_result *)(d + oRes);
  hipLaunchKernelGGL(k_mlpnp_points, dim3((n + 255) / 256), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_mlpnp_hypotheses, dim3((n_hyp + kMlpnpWaves - 1) / kMlpnpWaves), dim3(kMlpnpThreads), 0, c->stream, a);
  hipLaunchKernelGGL(k_mlpnp_select, dim3(1), dim3(256), 0, c->stream, a);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  if (nf > 0) memcpy(inlier, h + oIn, NF);
  memcpy(res, h + oRes, sizeof *res);
  if (hyp_inliers) memcpy(hyp_inliers, h + oCnt, H * 4);
  if (hyp_T) memcpy(hyp_T, h + oT, H * 96);
  return VSG_OK;
}

int vsg_mlpnp_ransac_parameters(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, int n,
                                int *min_inliers_out, int *max_its_out) {
  if (n < 0 || !min_inliers_out || !max_its_out) return VSG_ERR_INVALID;
  mlpnp::ransac_parameters(probability, min_inliers, max_iterations, min_set, epsilon, n, min_inliers_out, max_its_out);
  return VSG_OK;
}

int vsg_mlpnp_draw_sets(int n, int n_hyp, int (*random_int)(int lo, int hi, void *ctx), void *ctx, int32_t *sets) {
  if (n < mlpnp::kMinSet || n_hyp < 0 || !sets) return VSG_ERR_INVALID;
  std::vector<int32_t> all((size_t)n), avail;
  for (int i = 0; i < n; i++) all[(size_t)i] = i;
  for (int k = 0; k < n_hyp; k++) {
    avail = all;  // :125
    for (int i = 0; i < mlpnp::kMinSet; i++) {
      const int hi = (int)avail.size() - 1;
      int randi;
      if (random_int) {
        randi = random_int(0, hi, ctx);
      } else {  // Random.cpp:47-50
        const int dd = hi - 0 + 1;
        randi = (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * dd) + 0;
      }
      if (randi < 0 || randi > hi) return VSG_ERR_INVALID;
      sets[6 * (size_t)k + i] = avail[(size_t)randi];
      avail[(size_t)randi] = avail.back();
      avail.pop_back();
    }
  }
  return VSG_OK;
}

}  // extern "C"
