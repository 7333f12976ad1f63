// What a caller of the library does per frame WITHOUT resident map points (tools/local_points_probe.py, side A):
// Tracking::SearchLocalPoints' loop on the host -- Frame::isInFrustum per local map point (vsg_frustum.h compiled for the
// host: the same arithmetic the kernel runs), then the gather of the descriptors and flags that
// vsg_frame_search_by_projection takes per call.  Single thread, -O2.
#include <string.h>

#include "vsg_frustum.h"

extern "C" void lp_host_side(const vsg_frame_pose *pose, const float *bounds /* minX, minY, maxX, maxY */,
                             float viewing_cos_limit, int n, const int32_t *slots, const float *world_pos,
                             const float *normal, const float *min_dist, const float *max_dist, const uint8_t *desc,
                             const uint8_t *observed, uint8_t *in_view, float *proj_x, float *proj_y, float *proj_xr,
                             int32_t *scale_level, float *view_cos, uint8_t *q_desc, uint8_t *q_observed) {
  for (int i = 0; i < n; i++) {
    const int s = slots[i];
    const float *P = world_pos + 3 * s, *N = normal + 3 * s;
    const vsg::FrustumOut o = vsg::frustum_point(*pose, bounds[0], bounds[2], bounds[1], bounds[3], viewing_cos_limit,
                                                 P[0], P[1], P[2], N[0], N[1], N[2], min_dist[s], max_dist[s]);
    in_view[i] = (uint8_t)o.in_view, proj_x[i] = o.proj_x, proj_y[i] = o.proj_y, proj_xr[i] = o.proj_xr;
    scale_level[i] = o.scale_level, view_cos[i] = o.view_cos;
    memcpy(q_desc + 32 * (size_t)i, desc + 32 * (size_t)s, 32);
    q_observed[i] = observed[s];
  }
}
