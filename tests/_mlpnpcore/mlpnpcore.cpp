// Host build of csrc/vsg_mlpnp.h for the tests (tests/mlpnp_hostcore.py): the same source the kernels of vsg_mlpnp.hip
// compile, with -ffp-contract=off.
#include <vector>

#include "vsg_mlpnp.h"

using namespace vsg;

extern "C" {

int mc_sizes(int *point, int *pose, int *result) {
  *point = (int)sizeof(mlpnp::Point), *pose = (int)sizeof(mlpnp::Pose), *result = (int)sizeof(vsg_mlpnp_result);
  return mlpnp::kSweeps;
}
void mc_acos(int n, const double *x, double *y) {
  for (int i = 0; i < n; i++) y[i] = mlpnp::dacos(x[i]);
}
void mc_cbrt(int n, const double *x, double *y) {
  for (int i = 0; i < n; i++) y[i] = mlpnp::dcbrt(x[i]);
}
void mc_rot2rodrigues(const double *R, double *w) {
  const double M[3][3] = {{R[0], R[1], R[2]}, {R[3], R[4], R[5]}, {R[6], R[7], R[8]}};
  mlpnp::rot2rodrigues(M, w);
}
// the correspondences of the features with a slot, in feature order; returns how many
int mc_points(int n_feat, const int32_t *slots, const float *world_pos, const float *kx, const float *ky, const int32_t *octave,
              const float *cam, const float *level_sigma2, float th2, mlpnp::Point *pts) {
  const mlpnp::Camera c = {cam[0], cam[1], cam[2], cam[3]};
  int e = 0;
  for (int i = 0; i < n_feat; i++)
    if (slots[i] >= 0) pts[e++] = mlpnp::make_point(c, kx[i], ky[i], level_sigma2[octave[i]], th2, world_pos + 3 * (size_t)slots[i]);
  return e;
}
// every hypothesis of `sets`: T [12] = [R | t], info [8], the count and the flags [n]
void mc_hypotheses(int n, const mlpnp::Point *pts, const float *cam, int n_hyp, const int32_t *sets, double *T, double *info,
                   int32_t *counts, uint8_t *flags) {
  const mlpnp::Camera c = {cam[0], cam[1], cam[2], cam[3]};
  for (int k = 0; k < n_hyp; k++) {
    mlpnp::Pose P;
    mlpnp::hypothesis_host(pts, sets + 6 * (size_t)k, &P, info + 8 * (size_t)k);
    mlpnp::canon_pose(P, T + 12 * (size_t)k);
    int cnt = 0;
    for (int i = 0; i < n; i++) cnt += (flags[(size_t)k * n + i] = mlpnp::is_inlier(P, c, pts[i]) ? 1 : 0);
    counts[k] = cnt;
  }
}
// computePose over the set `member` (the solve Refine() runs and discards), the count and flags of that pose
void mc_refine(int n, const mlpnp::Point *pts, const float *cam, const uint8_t *member, double *T, double *info, int32_t *count,
               uint8_t *flags) {
  const mlpnp::Camera c = {cam[0], cam[1], cam[2], cam[3]};
  mlpnp::Pose P;
  mlpnp::member_pose_host(pts, member, n, &P, info);
  mlpnp::canon_pose(P, T);
  int cnt = 0;
  for (int i = 0; i < n; i++) cnt += (flags[i] = mlpnp::is_inlier(P, c, pts[i]) ? 1 : 0);
  *count = cnt;
}
void mc_select(const int32_t *counts, int first, int n_iterations, int max_its, int min_inliers, int32_t *out) {
  const mlpnp::Selection s = mlpnp::select(counts, first, n_iterations, max_its, min_inliers);
  out[0] = s.found, out[1] = s.no_more, out[2] = s.refined, out[3] = s.best, out[4] = s.iterations, out[5] = s.pose, out[6] = s.records;
}
// what vsg_frame_mlpnp_ransac refuses before it enqueues, the handles aside: 1 = the arguments pass; *n = correspondences
int mc_args_ok(int n_feat, const int32_t *slots, int capacity, const float *level_sigma2, int nlevels, const int32_t *octave, float th2,
               int min_inliers, int max_its, int first, int n_iterations, int n_hyp, const int32_t *sets, const uint8_t *inlier,
               const vsg_mlpnp_result *res, int *n) {
  if (!octave) return 0;
  return mlpnp::args_ok(n_feat, slots, capacity, level_sigma2, nlevels, [&](int i) { return octave[i]; }, th2, min_inliers, max_its,
                        first, n_iterations, n_hyp, sets, inlier, res, n) ? 1 : 0;
}
void mc_ransac(int n_feat, const int32_t *slots, const float *world_pos, const float *kx, const float *ky, const int32_t *octave,
               const float *cam, const float *level_sigma2, float th2, int min_inliers, int max_its, int first, int n_iterations,
               int n_hyp, const int32_t *sets, int n, uint8_t *inlier, vsg_mlpnp_result *res, int32_t *hyp_inliers, double *hyp_T) {
  const mlpnp::Camera c = {cam[0], cam[1], cam[2], cam[3]};
  std::vector<mlpnp::Point> pts((size_t)(n > 0 ? n : 1));
  mlpnp::ransac_host(n_feat, slots, world_pos, kx, ky, octave, c, level_sigma2, th2, min_inliers, max_its, first, n_iterations, n_hyp,
                     sets, n, pts.data(), inlier, res, hyp_inliers, hyp_T);
}
void mc_parameters(double probability, int min_inliers, int max_iterations, int min_set, float epsilon, int n, int *mi, int *its) {
  mlpnp::ransac_parameters(probability, min_inliers, max_iterations, min_set, epsilon, n, mi, its);
}

}  // extern "C"
