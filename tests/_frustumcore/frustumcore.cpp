// Host build of the product's logf restatement (vsg_math.h) and of Frame::isInFrustum for one point (vsg_frustum.h),
// for tests/test_frustum_hostmath.py: the same source the kernels compile, against libm and the NumPy reference.
#include <math.h>
#include <string.h>

#include "vsg_frustum.h"

static int level_of(float lg, float log_sf, int n_levels) {
  int s = vsg::cvt_int_x86(ceilf(lg / log_sf));
  if (s < 0)
    s = 0;
  else if (s >= n_levels)
    s = n_levels - 1;
  return s;
}

extern "C" {

float fc_logf(float x, int use_fma) { return use_fma ? vsg::logf_glibc<true>(x) : vsg::logf_glibc<false>(x); }
float fc_log_f32(float x) { return vsg::log_f32(x); }

// every float whose bit pattern lies in [lo_bits, hi_bits): counts[0] = values, counts[1] / counts[2] = bit mismatches of
// the uncontracted / FMA variant against libm's logf, counts[3 + k] = values whose predicted level differs for scale
// factor sf[k] (either variant); first[] = up to cap argument bit patterns of the first mismatches of any kind
void fc_logf_sweep(uint32_t lo_bits, uint32_t hi_bits, const float *sf, int nsf, int n_levels, long long *counts,
                   uint32_t *first, int cap) {
  float log_sf[8];
  for (int k = 0; k < nsf && k < 8; k++) log_sf[k] = logf(sf[k]);
  for (int k = 0; k < 3 + nsf; k++) counts[k] = 0;
  int shown = 0;
  for (uint32_t u = lo_bits; u < hi_bits; u++) {
    float x;
    memcpy(&x, &u, 4);
    const float ref = logf(x), a = vsg::logf_glibc<false>(x), b = vsg::logf_glibc<true>(x);
    bool bad = false;
    counts[0]++;
    if (vsg::f2u(ref) != vsg::f2u(a)) counts[1]++, bad = true;
    if (vsg::f2u(ref) != vsg::f2u(b)) counts[2]++, bad = true;
    // Equal bits give equal levels, so the levels are evaluated only where the bits differ.  The level counts are therefore
    // meaningful on their own only together with the mismatch counts: the test asserts both (0 mismatches expected; were
    // there any, these counts say whether one of them moves a level).
    if (bad)
      for (int k = 0; k < nsf && k < 8; k++) {
        const int lr = level_of(ref, log_sf[k], n_levels);
        if (lr != level_of(a, log_sf[k], n_levels) || lr != level_of(b, log_sf[k], n_levels)) counts[3 + k]++;
      }
    if (bad && shown < cap) first[shown++] = u;
  }
}

// vsg::frustum_point for n points: the arrays of vsg_frame_is_in_frustum
void fc_frustum(const vsg_frame_pose *pose, const float *bounds /* minX, minY, maxX, maxY */, float viewing_cos_limit,
                int n, const float *world_pos, const float *normal, const float *min_dist, const float *max_dist,
                uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr, float *depth, int32_t *scale_level,
                float *view_cos) {
  for (int i = 0; i < n; i++) {
    const float *P = world_pos + 3 * i, *N = normal + 3 * i;
    const vsg::FrustumOut o = vsg::frustum_point(*pose, bounds[0], bounds[2], bounds[1], bounds[3], viewing_cos_limit,
                                                 P[0], P[1], P[2], N[0], N[1], N[2], min_dist[i], max_dist[i]);
    in_view[i] = (uint8_t)o.in_view, proj_x[i] = o.proj_x, proj_y[i] = o.proj_y, proj_xr[i] = o.proj_xr;
    depth[i] = o.depth, scale_level[i] = o.scale_level, view_cos[i] = o.view_cos;
  }
}
}
