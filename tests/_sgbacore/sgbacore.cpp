// The host build of csrc/vsg_sgraph_ba.h behind a C interface (tests/test_sgba_hostmath.py through ctypes, sgba_sanitized.cpp
// as a program of its own): the argument check, the lists, the set-up, every phase in the device's order and tree, and the
// outs exactly as vsg_sgraph_ba.hip stages them, with the arrays the caller would otherwise hold on the device.
#include <cstring>

#include "vsg_sgraph_ba.h"

using namespace vsg;

extern "C" {

// Returns what vsg_mappoints_local_bundle_adjustment_sgraph returns.  The visual arguments are lbacore_run's
// (tests/_localbacore); the others are the entry's own.
int sgbacore_run(int capacity, float *store_pos, int n_points, const int32_t *slots, const int32_t *obs_off,
                 const int32_t *obs_kf, const int32_t *obs_idx, int n_kf, const int32_t *kf_off, const float *kx, const float *ky,
                 const int32_t *oct, const float *ur, const int32_t *nleft, const vsg_pose_se3 *kf_Tcw, const uint8_t *kf_fixed,
                 const vsg_ba_camera *kf_cam, const float *inv_level_sigma2, int nlevels, int iterations,
                 const volatile uint8_t *stop_flag, vsg_pose_se3d *kf_Tcw_out, float *world_pos_out, uint8_t *erase,
                 double *chi2, int n_planes, const double *plane_eq, const int32_t *pl_obs_off, const int32_t *pl_obs_kf,
                 const double *pl_obs_local, const double *pl_obs_G, const double *w_plane_kf, const double *w_plane_point,
                 int n_rooms, const double *room_center, const int32_t *room_n_walls, const int32_t *room_wall,
                 double *plane_eq_out, double *room_center_out, uint8_t *erase_plane, double *chi2_plane_kf,
                 double *chi2_plane_point, vsg_sgraph_local_ba_result *res) {
  if (!store_pos || n_kf < 0 || !inv_level_sigma2 || !kf_Tcw_out || !erase || !res) return VSG_ERR_INVALID;
  if (n_kf > 0 && (!kf_off || !kf_Tcw || !kf_fixed || !kf_cam)) return VSG_ERR_INVALID;
  const sgba::SemIn in = {n_planes, plane_eq, pl_obs_off, pl_obs_kf, pl_obs_local, pl_obs_G, w_plane_kf, w_plane_point,
                          n_rooms,  room_center, room_n_walls, room_wall};
  if ((n_planes > 0 && !plane_eq_out) || (n_rooms > 0 && !room_center_out)) return VSG_ERR_INVALID;
  if (n_planes > 0 && pl_obs_off && pl_obs_off[0] == 0 && pl_obs_off[n_planes] > 0 && !erase_plane) return VSG_ERR_INVALID;
  std::vector<int32_t> kf_n((size_t)n_kf);
  for (int k = 0; k < n_kf; k++) kf_n[(size_t)k] = kf_off[k + 1] - kf_off[k];
  sgba::HostRun run;
  lba::Topology &T = run.V.T;
  int ran = 0;
  const int rc = sgba::check_and_build(
      n_points, slots, obs_off, obs_kf, obs_idx, n_kf, kf_n.data(), nleft, [&](int k, int i) { return (int)oct[kf_off[k] + i]; },
      kf_fixed, capacity, nlevels, iterations, stop_flag, in, &T, &run.ST, &ran);
  if (rc != VSG_OK) return rc;
  if (!ran) {
    if (n_points == 0) T.n_fixed = T.n_opt = 0;
    sgba::fill_result(res, T, nullptr, nullptr);
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
  run.setup(pos.data(), ex.data(), ey.data(), eur.data(), eoct.data(), kf_Tcw, kf_fixed, kf_cam, inv_level_sigma2, nlevels, iterations, in);
  run.run(stop_flag);
  std::vector<double> c2(E);
  run.V.outputs(kf_Tcw, pos.data(), kf_Tcw_out, pos_out.data(), erase, c2.data());
  if (chi2 && E) memcpy(chi2, c2.data(), E * 8);
  for (size_t i = 0; i < P; i++)
    if (obs_off[i] != obs_off[i + 1])
      for (int d = 0; d < 3; d++) store_pos[3 * (size_t)slots[i] + d] = pos_out[3 * i + d];
  if (world_pos_out) memcpy(world_pos_out, pos_out.data(), P * 12);
  run.outputs(in, plane_eq_out, room_center_out, erase_plane, chi2_plane_kf, chi2_plane_point);
  sgba::fill_result(res, T, &run.ST, &run.V.S);
  int n_erase = 0, n_erase_plane = 0;
  for (size_t e = 0; e < E; e++) n_erase += erase[e] != 0;
  for (int o = 0; o < run.ST.n_obs; o++) n_erase_plane += erase_plane[o] != 0;
  res->local.n_erase = n_erase, res->n_erase_plane = n_erase_plane;
  return VSG_OK;
}

// the written-out functions by themselves
double sgbacore_atan2(double y, double x) { return sgba::datan2(y, x); }
void sgbacore_sincos(double x, double *s, double *c) { sgba::dsincos(x, s, c); }
void sgbacore_plane_oplus(const double *c, const double *v, double *o) { sgba::plane_oplus(c, v, o); }
void sgbacore_plane_ominus(const double *a, const double *b, double *e) { sgba::plane_ominus(a, b, e); }
void sgbacore_plane_transform(const double *q, const double *t, const double *c, double *o) {
  pose::Est T;
  for (int k = 0; k < 4; k++) T.q[k] = q[k];
  for (int k = 0; k < 3; k++) T.t[k] = t[k];
  sgba::plane_transform(T, c, o);
}
double sgbacore_point_plane_error(const double *q, const double *t, const double *Pj, const double *G) {
  pose::Est T;
  for (int k = 0; k < 4; k++) T.q[k] = q[k];
  for (int k = 0; k < 3; k++) T.t[k] = t[k];
  return sgba::point_plane_error(T, Pj, G);
}
void sgbacore_wall_pair(const double *a, const double *b, double *v) { sgba::wall_pair(a, b, v); }
}
