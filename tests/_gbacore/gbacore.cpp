// The host build of csrc/vsg_global_ba.h behind a C interface (tests/test_gba_hostmath.py through ctypes, gba_sanitized.cpp as
// a program of its own): the argument check, the lists, the set-up, every phase in the device's order and tree, the blocked
// reduced solve, and the outs exactly as vsg_global_ba.hip stages them, with the arrays the caller would otherwise hold on
// the device.
#include <cstring>

#include "vsg_global_ba.h"

using namespace vsg;

namespace {
// gbacore_stop_after: the flag of the next gbacore_run is set at the look behind that many iterations (0: never), as a second
// thread's store landing there would
thread_local int t_stop_after = 0;
struct Look {
  volatile uint8_t *flag;
  int after;
};
void set_flag_at_look(void *ctx, int it) {
  Look *l = (Look *)ctx;
  if (it + 1 == l->after) *l->flag = 1;
}
}  // namespace

extern "C" {

void gbacore_stop_after(int iterations) { t_stop_after = iterations; }

// Returns what vsg_mappoints_global_bundle_adjustment returns.  The store is store_pos[3 * capacity] (its world_pos, written
// as the device writes it); keyframe k's features are [kf_off[k], kf_off[k + 1]) of kx / ky / oct / ur; nleft[k] = Nleft.
int gbacore_run(int capacity, float *store_pos, int n_points, const int32_t *slots, const int32_t *obs_off,
                const int32_t *obs_kf, const int32_t *obs_idx, int n_kf, const int32_t *kf_off, const float *kx, const float *ky,
                const int32_t *oct, const float *ur, const int32_t *nleft, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed,
                const vsg_ba_camera *kf_cam, const float *inv_level_sigma2, int nlevels, int iterations, int robust,
                int write_store, const volatile uint8_t *stop_flag, vsg_pose_se3d *kf_Tcw_out, float *world_pos_out,
                uint8_t *included, double *chi2, vsg_global_ba_result *res) {
  if (!store_pos || n_kf < 0 || !inv_level_sigma2 || !kf_Tcw_out || !included || !res) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kf_off || !kf_Tcw || !kf_fixed || !kf_cam)) return VSG_ERR_INVALID;
  std::vector<int32_t> kf_n((size_t)n_kf);
  for (int k = 0; k < n_kf; k++) kf_n[(size_t)k] = kf_off[k + 1] - kf_off[k];
  lba::Topology T;
  int ran = 0;
  const int rc = gba::check_and_build(
      n_points, slots, obs_off, obs_kf, obs_idx, n_kf, kf_n.data(), nleft, [&](int k, int i) { return (int)oct[kf_off[k] + i]; },
      kf_fixed, capacity, nlevels, iterations, robust, write_store, world_pos_out, stop_flag, &T, &ran);
  if (rc != VSG_OK) return rc;
  if (n_points > 0) gba::fill_included(included, n_points, obs_off);
  if (!ran) {
    if (n_points == 0) T.n_fixed = T.n_opt = 0;
    gba::fill_result(res, T, nullptr);
    return VSG_OK;
  }
  const size_t E = (size_t)T.E, P = (size_t)T.P;
  std::vector<float> ex(E), ey(E), eur(E), pos(3 * P), pos_out(3 * P);
  std::vector<int32_t> eoct(E);
  for (size_t e = 0; e < E; e++) {
    const size_t f = (size_t)kf_off[T.e_kf[e]] + (size_t)T.e_idx[e];
    ex[e] = kx[f], ey[e] = ky[f], eoct[e] = oct[f], eur[e] = ur ? ur[f] : -1.0f;
  }
  for (size_t i = 0; i < P; i++)
    for (int d = 0; d < 3; d++) pos[3 * i + d] = store_pos[3 * (size_t)slots[i] + d];
  gba::HostRun run;
  run.T = T, run.kernel.robust = robust;
  Look look{const_cast<volatile uint8_t *>(stop_flag), t_stop_after};
  if (stop_flag && t_stop_after > 0) run.at_look = set_flag_at_look, run.look_ctx = &look;
  t_stop_after = 0;
  run.setup(pos.data(), ex.data(), ey.data(), eur.data(), eoct.data(), kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, nlevels, iterations);
  run.run(stop_flag);
  run.outputs(kf_Tcw, pos.data(), kf_Tcw_out, pos_out.data(), chi2);
  if (write_store)
    for (size_t i = 0; i < P; i++)
      if (obs_off[i] != obs_off[i + 1])
        for (int d = 0; d < 3; d++) store_pos[3 * (size_t)slots[i] + d] = pos_out[3 * i + d];
  if (world_pos_out) memcpy(world_pos_out, pos_out.data(), P * 12);
  gba::fill_result(res, T, &run.S);
  return VSG_OK;
}

// the two reduced solves on a copy of M (n x n row-major, the lower triangle): lba::solve_reduced_host and the blocked schedule
int gbacore_solve(int blocked, int n, const double *M, const double *b, double *x) {
  std::vector<double> A(M, M + (size_t)n * (size_t)n);
  return (blocked ? gba::solve_reduced_blocked_host(n, A.data(), b, x) : lba::solve_reduced_host(n, A.data(), b, x)) ? 1 : 0;
}

void gbacore_geometry(int *panel, int *tile, int *max_opt_kf) { *panel = gba::kPanel, *tile = gba::kTile, *max_opt_kf = gba::kMaxOptKf; }
}
