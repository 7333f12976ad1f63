// The host build of csrc/vsg_pose_opt.h behind a C interface (tests/test_pose_hostmath.py through ctypes,
// pose_sanitized.cpp as a program of its own): the argument check, the gather, the rounds and the copy-out exactly as
// vsg_pose.hip stages them, with the arrays the caller would otherwise have uploaded.
#include <cmath>
#include <cstring>

#include "vsg_pose_opt.h"

using namespace vsg;

extern "C" {

// Returns nInitialCorrespondences - nBad, or -6 (VSG_ERR_INVALID).  pose7 = q x y z w, t; cam5 = fx fy cx cy bf.
// hold_round == 2: the call stops after round 2's optimize (held_qt = the estimate then, may be NULL), `removed` is
// applied and the call resumes, as vsg_frame_pose_optimization + _resume do.  res_qt[7], res_i = {n_initial, n_bad,
// rounds_run, held at the hold}.
int posecore_run(int n, const int32_t *feat_slots, int capacity, const float *world_pos, const float *kx, const float *ky,
                 const int32_t *octave, const float *u_right, const float *pose7, const float *cam5,
                 const float *inv_level_sigma2, int nlevels, int hold_round, const uint8_t *removed, uint8_t *outlier,
                 float *chi2, double *res_qt, int32_t *res_i, double *held_qt) {
  if (!feat_slots || !pose7 || !cam5 || !inv_level_sigma2 || !res_qt || !res_i || !outlier) return -6;
  if (nlevels < 1 || nlevels > 16 || (hold_round != -1 && hold_round != 2)) return -6;
  int E = 0;
  if (!pose::check_slots(n, feat_slots, capacity, nlevels, n, [&](int i) { return octave[i]; }, &E)) return -6;
  const pose::Est input = pose::est_from_pose(pose7, pose7 + 4);
  res_i[0] = E, res_i[1] = res_i[2] = res_i[3] = 0;
  if (E < 3) {
    for (int i = 0; i < n; i++)
      if (feat_slots[i] >= 0) outlier[i] = 0;
    for (int k = 0; k < 4; k++) res_qt[k] = input.q[k];
    for (int k = 0; k < 3; k++) res_qt[4 + k] = input.t[k];
    return 0;
  }
  pose::HostCall call;
  const pose::Cam cam = {(double)cam5[0], (double)cam5[1], (double)cam5[2], (double)cam5[3], (double)cam5[4]};
  call.gather(n, feat_slots, world_pos, kx, ky, octave, u_right, inv_level_sigma2, nlevels, cam, input);
  call.rounds(hold_round == 2 ? pose::kModeHold : pose::kModeAll);
  if (call.ctl.held) {
    res_i[3] = 1;
    if (held_qt) {
      for (int k = 0; k < 4; k++) held_qt[k] = pose::canon(call.ctl.est.q[k]);
      for (int k = 0; k < 3; k++) held_qt[4 + k] = pose::canon(call.ctl.est.t[k]);
    }
    call.remove(removed);
    call.rounds(pose::kModeResume);
  }
  call.copy_out(outlier, chi2);
  for (int k = 0; k < 4; k++) res_qt[k] = pose::canon(call.ctl.est.q[k]);
  for (int k = 0; k < 3; k++) res_qt[4 + k] = pose::canon(call.ctl.est.t[k]);
  res_i[1] = call.ctl.n_bad, res_i[2] = call.ctl.rounds_run;
  return E - call.ctl.n_bad;
}

void posecore_sincos(int n, const double *x, double *s, double *c) {
  for (int i = 0; i < n; i++) pose::sincos_pose(x[i], &s[i], &c[i]);
}

// est_oplus alone (the tiny-angle branch and the update's normalisation): est7 = q, t; update6 = omega, upsilon
void posecore_oplus(const double *est7, const double *update6, double *out7) {
  pose::Est e;
  memcpy(e.q, est7, 32), memcpy(e.t, est7 + 4, 24);
  const pose::Est o = pose::est_oplus(e, update6);
  memcpy(out7, o.q, 32), memcpy(out7 + 4, o.t, 24);
}
}
