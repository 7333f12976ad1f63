// Host build of Sim3Solver's arithmetic (vsg_sim3.h), for tests/sim3_hostcore.py: the same source the kernels of
// vsg_sim3.hip compile, against the NumPy restatement and against the device.
#include "vsg_sim3.h"

#include <vector>

using namespace vsg;

extern "C" {

int sc_sizes(int *point, int *result) {
  *point = (int)sizeof(sim3::Point), *result = (int)sizeof(vsg_sim3_result);
  return sim3::kSweeps;
}

// the eigenvector of the largest eigenvalue of n symmetric 4 x 4 float matrices (double, before any rounding)
void sc_eigenvectors(int n, const float *N, double *q) {
  for (int i = 0; i < n; i++) sim3::largest_eigenvector(N + 16 * (size_t)i, q + 4 * (size_t)i);
}

void sc_rotations(int n, const double *q, float *R) {
  for (int i = 0; i < n; i++) sim3::rotation_from_quaternion(q + 4 * (size_t)i, R + 9 * (size_t)i);
}

// the set-up of n correspondences: pts = n x sim3::Point (12 floats)
void sc_points(int n, const vsg_frame_pose *kf1, const vsg_frame_pose *kf2, const float *Xw1, const float *Xw2, const float *max_err1,
               const float *max_err2, float *pts) {
  static_assert(sizeof(sim3::Point) == 48, "Point is 12 floats");
  for (int i = 0; i < n; i++)
    ((sim3::Point *)pts)[i] = sim3::make_point(*kf1, *kf2, Xw1 + 3 * (size_t)i, Xw2 + 3 * (size_t)i, max_err1[i], max_err2[i]);
}

// n_hyp hypotheses of given triples: hyp = n_hyp x {R12[9], t12[3], s12, T12[16], T21[16]} (45 floats), N = n_hyp x 16,
// err = n_hyp x n x 2 and flags = n_hyp x n (either may be NULL)
void sc_hypotheses(int n, const float *pts, const vsg_frame_pose *kf1, const vsg_frame_pose *kf2, int fix_scale, int n_hyp,
                   const int32_t *samples, float *hyp, float *N, float *err, uint8_t *flags) {
  static_assert(sizeof(sim3::Hypothesis) == 180, "Hypothesis is 45 floats");
  const sim3::Point *P = (const sim3::Point *)pts;
  const sim3::Camera cam1 = sim3::camera_of(*kf1), cam2 = sim3::camera_of(*kf2);
  for (int k = 0; k < n_hyp; k++) {
    const sim3::Point &a = P[samples[3 * k]], &b = P[samples[3 * k + 1]], &c = P[samples[3 * k + 2]];
    float P1[9], P2[9];
    for (int r = 0; r < 3; r++) {
      P1[r] = a.X1[r], P1[3 + r] = b.X1[r], P1[6 + r] = c.X1[r];
      P2[r] = a.X2[r], P2[3 + r] = b.X2[r], P2[6 + r] = c.X2[r];
    }
    const sim3::Hypothesis h = sim3::compute_sim3(P1, P2, fix_scale != 0, N + 16 * (size_t)k);
    ((sim3::Hypothesis *)hyp)[k] = h;
    for (int i = 0; i < n; i++) {
      float e[2];
      const bool in = sim3::is_inlier(h, cam1, cam2, P[i], e);
      if (err) err[2 * ((size_t)k * n + i)] = e[0], err[2 * ((size_t)k * n + i) + 1] = e[1];
      if (flags) flags[(size_t)k * n + i] = in ? 1 : 0;
    }
  }
}

void sc_select(const int32_t *counts, int n_hyp, int min_inliers, int32_t *out) {
  const sim3::Selection s = sim3::select(counts, n_hyp, min_inliers);
  out[0] = s.best, out[1] = s.converged, out[2] = s.iterations;
}

// what vsg_mappoints_sim3_ransac refuses before it enqueues, the handles aside: 1 = the arguments pass
int sc_args_ok(int n, const int32_t *slots1, const int32_t *slots2, int capacity1, int capacity2, const float *max_err1,
               const float *max_err2, int min_inliers, int n_hyp, const int32_t *samples, const uint8_t *inlier) {
  return sim3::args_ok(n, slots1, slots2, max_err1, max_err2, min_inliers, n_hyp, samples, inlier) &&
                 sim3::slots_ok(n, slots1, capacity1) && sim3::slots_ok(n, slots2, capacity2)
             ? 1
             : 0;
}

// the whole call on positions the caller holds (sim3::ransac_host); hyp_inliers / hyp_T12 may be NULL
void sc_ransac(int n, const float *Xw1, const float *Xw2, const float *max_err1, const float *max_err2, const vsg_frame_pose *kf1,
               const vsg_frame_pose *kf2, int fix_scale, int min_inliers, int n_hyp, const int32_t *samples, int early_exit,
               uint8_t *inlier, vsg_sim3_result *res, int32_t *hyp_inliers, float *hyp_T12) {
  std::vector<sim3::Point> pts((size_t)n);
  std::vector<int32_t> counts((size_t)n_hyp);
  sim3::ransac_host(n, Xw1, Xw2, max_err1, max_err2, *kf1, *kf2, fix_scale != 0, min_inliers, n_hyp, samples, early_exit != 0,
                    pts.data(), counts.data(), inlier, res, hyp_inliers, hyp_T12);
}
}
