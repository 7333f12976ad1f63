// The host build of csrc/vsg_sim3_opt.h behind a C interface (tests/test_sim3opt_hostmath.py through ctypes,
// sim3opt_sanitized.cpp as a program of its own): the argument check, the gather, both optimisations with their checks
// and the copy-out exactly as vsg_sim3_opt.hip stages them, with the arrays the caller would otherwise have uploaded.
#include <cmath>
#include <cstring>

#include "vsg_sim3_opt.h"

using namespace vsg;

extern "C" {

// Returns what vsg_frame_optimize_sim3 returns, or -6 (VSG_ERR_INVALID).  n1 / n2 = the keyframes' feature counts; k1 /
// k2 = x, y per feature; pos1 / pos2 = the stores' positions, cap1 / cap2 slots each.  fix_scale bit 1 (value 2) is the
// test-only FIRST_FRESH variant of sim3opt::run: NOT the reference, it recomputes the errors at the first check.
int sim3optcore_run(int n1, int n2, const int32_t *slots1, const int32_t *slots2, const int32_t *idx2, const int32_t *level2,
                    int cap1, int cap2, const float *pos1, const float *pos2, const float *k1x, const float *k1y,
                    const int32_t *oct1, const float *k2x, const float *k2y, const int32_t *oct2, const vsg_frame_pose *pose1,
                    const vsg_frame_pose *pose2, const float *sig1, const float *sig2, int nlevels, const vsg_sim3d *S12,
                    float th2, int fix_scale, int all_points, uint8_t *state, double *chi2, vsg_sim3_opt_result *res) {
  if (!slots1 || !slots2 || !idx2 || !level2 || !pose1 || !pose2 || !sig1 || !sig2 || !S12 || !state || !res) return -6;
  if (nlevels < 1 || nlevels > 16 || !sim3opt::th2_ok(th2)) return -6;
  int n_cand = 0;
  if (!sim3opt::check_entries(n1, slots1, slots2, idx2, level2, cap1, cap2, n2, nlevels, all_points != 0,
                              [&](int i) { return (int)oct1[i]; }, [&](int i) { return (int)oct2[i]; }, &n_cand))
    return -6;
  if (n_cand == 0) {
    for (int i = 0; i < n1; i++) state[i] = sim3opt::kNoEdge;
    sim3opt::fill_result(res, *S12, sim3opt::Counts{0, 0, 0}, 0, 0, 5, 0);
    return 0;
  }
  sim3opt::HostCall call;
  call.gather(n1, slots1, slots2, idx2, level2, pos1, pos2, k1x, k1y, oct1, k2x, k2y, oct2, *pose1, *pose2, sig1, sig2,
              nlevels, all_points != 0);
  const sim3opt::Outcome o = call.optimise(*pose1, *pose2, sim3opt::sim3_of(*S12), th2, (fix_scale & 1) != 0, (fix_scale & 2) != 0);
  call.copy_out(n1, state, chi2);
  sim3opt::fill_result(res, o.updated ? sim3opt::sim3d_canon(o.S12) : *S12, call.counts, o.n_bad, o.n_in, o.more_iterations,
                       o.updated);
  return o.ret;
}

void sim3optcore_exp(int n, const double *x, double *y) {
  for (int i = 0; i < n; i++) y[i] = sim3opt::exp_sim3(x[i]);
}

// sim3_exp, sim3_mul, sim3_inverse, sim3_map alone: 8 doubles per Sim3 (q, t, s)
static sim3opt::Sim3 load(const double *p) {
  sim3opt::Sim3 s;
  memcpy(s.q, p, 32), memcpy(s.t, p + 4, 24), s.s = p[7];
  return s;
}
static void store(const sim3opt::Sim3 &s, double *p) { memcpy(p, s.q, 32), memcpy(p + 4, s.t, 24), p[7] = s.s; }
void sim3optcore_exp7(const double *update7, double *out8) { store(sim3opt::sim3_exp(update7), out8); }
void sim3optcore_mul(const double *a8, const double *b8, double *out8) { store(sim3opt::sim3_mul(load(a8), load(b8)), out8); }
void sim3optcore_inverse(const double *a8, double *out8) { store(sim3opt::sim3_inverse(load(a8)), out8); }
void sim3optcore_map(const double *a8, const double *x3, double *out3) { sim3opt::sim3_map(load(a8), x3, out3); }
// oplusImpl: update7 is the CALLER'S array (fix_scale zeroes its entry 6)
void sim3optcore_oplus(const double *a8, double *update7, int fix_scale, double *out8) {
  store(sim3opt::sim3_oplus(load(a8), update7, fix_scale != 0), out8);
}
}
