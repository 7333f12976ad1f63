// vsg_sim3.hip -- Sim3Solver on resident map points (Sim3Solver.cc; LoopClosing.cc:678-690): vsg_mappoints_sim3_ransac, and
// the two host-only pieces of the solver's set-up, vsg_sim3_ransac_iterations and vsg_sim3_draw_samples.
//
// Three kernels back to back on the calling thread's stream, one wait:
//   k_sim3_points      one lane per correspondence: both positions out of the stores through the two poses, their images
//                      (vsg::sim3::make_point) into the calling thread's device arena -- the arena, not a buffer of the
//                      store, so that two threads may solve on one store at the same time;
//   k_sim3_hypotheses  one WAVE per hypothesis, kSim3Waves per workgroup: the Horn solve runs on every lane on identical
//                      bits (uniform control flow, nothing broadcast, as k_pose_optimize), the 64 lanes stride over the
//                      correspondences and the count is the popcount of the ballot, accumulated per wave -- an integer,
//                      independent of order.  No barrier: a wave past n_hyp leaves;
//   k_sim3_select      one workgroup: the counts into LDS, sim3::select over them by every lane (uniform), the chosen
//                      hypothesis recomputed, its flags and the result written.
// No inlier matrix is stored, no atomics, no grid-wide barrier, nothing spins; every loop is bounded by an argument or by
// sim3::kSweeps.  All stores are plain vector stores.
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <vector>

#include "vsg_frame_int.h"
#include "vsg_sim3.h"

using namespace vsg;

namespace {

enum { kSim3Waves = 4, kSim3Threads = 64 * kSim3Waves, kSelectThreads = 256 };

struct Sim3Args {
  const float *pos1, *pos2;         // the stores' GetWorldPos()
  const int *slots1, *slots2;       // [n]
  const float *max_err1, *max_err2; // [n]
  const int *samples;               // [3 * n_hyp]
  vsg_frame_pose kf1, kf2;
  int n, n_hyp, fix_scale, min_inliers;
  sim3::Point *pts;                 // [n], device arena
  int *counts;                      // [n_hyp], device arena
  int *hyp_inliers;                 // [n_hyp], the caller's copy of counts
  float *hyp_T12;                   // [16 * n_hyp] or nullptr
  uint8_t *inlier;                  // [n]
  vsg_sim3_result *res;
};

__global__ __launch_bounds__(256) void k_sim3_points(Sim3Args a) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= a.n) return;
  const size_t s1 = (size_t)a.slots1[i], s2 = (size_t)a.slots2[i];  // inside their stores: the host checked
  const float X1[3] = {a.pos1[3 * s1], a.pos1[3 * s1 + 1], a.pos1[3 * s1 + 2]};
  const float X2[3] = {a.pos2[3 * s2], a.pos2[3 * s2 + 1], a.pos2[3 * s2 + 2]};
  a.pts[i] = sim3::make_point(a.kf1, a.kf2, X1, X2, a.max_err1[i], a.max_err2[i]);
}

// the hypothesis of triple k, on every lane that asks
__device__ __forceinline__ sim3::Hypothesis hypothesis_k(const Sim3Args &a, int k) {
  const int i0 = a.samples[3 * k], i1 = a.samples[3 * k + 1], i2 = a.samples[3 * k + 2];  // inside [0, n): the host checked
  return sim3::hypothesis_of(a.pts[i0], a.pts[i1], a.pts[i2], a.fix_scale != 0);
}

__global__ __launch_bounds__(kSim3Threads) void k_sim3_hypotheses(Sim3Args a) {
  const int lane = threadIdx.x & 63, k = blockIdx.x * kSim3Waves + (threadIdx.x >> 6);
  if (k >= a.n_hyp) return;  // wave-uniform
  const sim3::Hypothesis h = hypothesis_k(a, k);
  const sim3::Camera cam1 = sim3::camera_of(a.kf1), cam2 = sim3::camera_of(a.kf2);
  int count = 0;
  for (int base = 0; base < a.n; base += 64) {  // wave-uniform trip count: every lane reaches the ballot
    const int i = base + lane;
    const bool in = i < a.n && sim3::is_inlier(h, cam1, cam2, a.pts[i < a.n ? i : 0], nullptr);
    count += __popcll(__ballot(in));
  }
  if (lane == 0) a.counts[k] = count;
  if (a.hyp_T12) {  // entry `lane` by selects: an index that varies by lane would put h into scratch
    float v = 0.0f;
#pragma unroll
    for (int j = 0; j < 16; j++) v = lane == j ? h.T12[j] : v;
    if (lane < 16) a.hyp_T12[16 * (size_t)k + lane] = sim3::canonf(v);
  }
}

__global__ __launch_bounds__(kSelectThreads) void k_sim3_select(Sim3Args a) {
  __shared__ int s_counts[sim3::kMaxHypotheses];
  for (int k = threadIdx.x; k < a.n_hyp; k += kSelectThreads) {
    const int c = a.counts[k];
    s_counts[k] = c, a.hyp_inliers[k] = c;
  }
  __syncthreads();
  const sim3::Selection s = sim3::select(s_counts, a.n_hyp, a.min_inliers);
  const sim3::Hypothesis h = hypothesis_k(a, s.best);
  const sim3::Camera cam1 = sim3::camera_of(a.kf1), cam2 = sim3::camera_of(a.kf2);
  for (int i = threadIdx.x; i < a.n; i += kSelectThreads) a.inlier[i] = sim3::is_inlier(h, cam1, cam2, a.pts[i], nullptr) ? 1 : 0;
  if (threadIdx.x == 0) sim3::fill_result(h, s, s_counts[s.best], a.res);
}

// (int)v of a double as the reference's x86-64 build converts it (cvttsd2si)
int cvt_int_x86_d(double v) { return (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : (int)0x80000000; }

}  // namespace

extern "C" {

int vsg_mappoints_sim3_ransac(vsg_mappoints *mp1, vsg_mappoints *mp2, int n, const int32_t *slots1, const int32_t *slots2,
                              const float *max_err1, const float *max_err2, const vsg_frame_pose *kf1,
                              const vsg_frame_pose *kf2, int fix_scale, int min_inliers, int n_hyp, const int32_t *samples,
                              uint8_t *inlier, vsg_sim3_result *res, int32_t *hyp_inliers, float *hyp_T12) {
  StoreView S1, S2;
  if (!store_view(mp1, &S1) || !store_view(mp2, &S2) || S1.device != S2.device || !kf1 || !kf2 || !res) return VSG_ERR_INVALID;
  if (!sim3::args_ok(n, slots1, slots2, max_err1, max_err2, min_inliers, n_hyp, samples, inlier)) return VSG_ERR_INVALID;
  if (!sim3::slots_ok(n, slots1, S1.capacity) || !sim3::slots_ok(n, slots2, S2.capacity)) return VSG_ERR_INVALID;
  // ---- nothing is refused from here on
  if (n < min_inliers) {  // :222-226
    if (n > 0) memset(inlier, 0, (size_t)n);
    sim3::fill_no_more(res);
    return VSG_OK;
  }
  int rc = VSG_OK;
  ThreadCtx *c = thread_ctx(S1.device, &rc);
  if (!c) return rc;
  const size_t N = (size_t)n, H = (size_t)n_hyp;
  Stage st;
  const size_t oS1 = st.add(N * 4), oS2 = st.add(N * 4), oE1 = st.add(N * 4), oE2 = st.add(N * 4), oSm = st.add(H * 12);
  const size_t oIn = st.add(N), oRes = st.add(sizeof(vsg_sim3_result)), oCnt = st.add(H * 4), oT = st.add(hyp_T12 ? H * 64 : 0);
  const size_t dev_pts = (N * sizeof(sim3::Point) + 63) & ~(size_t)63;
  rc = ctx_reserve(c, st.total, dev_pts + H * 4);
  if (rc != VSG_OK) return rc;
  uint8_t *h = c->h_pin, *d = c->d_pin;
  memcpy(h + oS1, slots1, N * 4), memcpy(h + oS2, slots2, N * 4);
  memcpy(h + oE1, max_err1, N * 4), memcpy(h + oE2, max_err2, N * 4), memcpy(h + oSm, samples, H * 12);
  Sim3Args a;
  memset(&a, 0, sizeof a);
  a.pos1 = S1.pos, a.pos2 = S2.pos;
  a.slots1 = (const int *)(d + oS1), a.slots2 = (const int *)(d + oS2);
  a.max_err1 = (const float *)(d + oE1), a.max_err2 = (const float *)(d + oE2), a.samples = (const int *)(d + oSm);
  a.kf1 = *kf1, a.kf2 = *kf2;
  a.n = n, a.n_hyp = n_hyp, a.fix_scale = fix_scale ? 1 : 0, a.min_inliers = min_inliers;
  a.pts = (sim3::Point *)c->d_buf, a.counts = (int *)(c->d_buf + dev_pts);
  a.hyp_inliers = (int *)(d + oCnt), a.hyp_T12 = hyp_T12 ? (float *)(d + oT) : nullptr;
  a.inlier = d + oIn, a.res = (vsg_sim3_result *)(d + oRes);
  hipLaunchKernelGGL(k_sim3_points, dim3((n + 255) / 256), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL(k_sim3_hypotheses, dim3((n_hyp + kSim3Waves - 1) / kSim3Waves), dim3(kSim3Threads), 0, c->stream, a);
  hipLaunchKernelGGL(k_sim3_select, dim3(1), dim3(kSelectThreads), 0, c->stream, a);
  const hipError_t launched = hipGetLastError(), waited = hipStreamSynchronize(c->stream);  // an error still waits
  if (launched != hipSuccess || waited != hipSuccess) return VSG_ERR_HIP;
  memcpy(inlier, h + oIn, N), memcpy(res, h + oRes, sizeof *res);
  if (hyp_inliers) memcpy(hyp_inliers, h + oCnt, H * 4);
  if (hyp_T12) memcpy(hyp_T12, h + oT, H * 64);
  return VSG_OK;
}

int vsg_sim3_ransac_iterations(double probability, int min_inliers, int max_iterations, int n) {
  if (n < 0 || min_inliers < 0) return VSG_ERR_INVALID;
  const float epsilon = (float)min_inliers / n;  // :131
  int nIterations;
  if (min_inliers == n)
    nIterations = 1;
  else  // :139: pow(float, int) and both logs are double
    nIterations = cvt_int_x86_d(std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3))));
  const int capped = nIterations < max_iterations ? nIterations : max_iterations;
  return capped > 1 ? capped : 1;
}

int vsg_sim3_draw_samples(int n, int n_hyp, int (*random_int)(int lo, int hi, void *ctx), void *ctx, int32_t *samples) {
  if (n < 3 || n_hyp < 0 || !samples) return VSG_ERR_INVALID;
  std::vector<int32_t> all((size_t)n), avail;
  for (int i = 0; i < n; i++) all[(size_t)i] = i;
  for (int k = 0; k < n_hyp; k++) {
    avail = all;  // :242
    for (int i = 0; i < 3; i++) {
      const int hi = (int)avail.size() - 1;
      int randi;
      if (random_int) {
        randi = random_int(0, hi, ctx);
      } else {  // Random.cpp:47-50
        const int dd = hi - 0 + 1;
        randi = (int)(((double)rand() / ((double)RAND_MAX + 1.0)) * dd) + 0;
      }
      if (randi < 0 || randi > hi) return VSG_ERR_INVALID;
      samples[3 * (size_t)k + i] = avail[(size_t)randi];
      avail[(size_t)randi] = avail.back();
      avail.pop_back();
    }
  }
  return VSG_OK;
}

}  // extern "C"
