// The caller-side half of Fuse(pKF, vpMapPoints, th) without resident map points, for tools/keyframe_points_probe.py: the
// per-point loop of ORBmatcher.cc:1194-1241 on the host (the kernel's own arithmetic, visual_sgraphs_amd/csrc/vsg_project.h,
// compiled -O2, one thread) and the gather of what vsg_frame_fuse takes, compacted to the projected points.
#include <string.h>

#include "vsg_project.h"

extern "C" int kp_host_side(const vsg_frame_pose *pose, const float *bounds /* minX, minY, maxX, maxY */, int n,
                            const uint8_t *skip, const float *world_pos, const float *normal, const float *min_dist,
                            const float *max_dist, const uint8_t *desc, float th, const float *scale_factors,
                            int32_t *index, uint8_t *q_desc, float *u, float *v, float *ur, float *radius,
                            int32_t *level) {
  const vsg::ImageBounds kf = vsg::keyframe_bounds({bounds[0], bounds[2], bounds[1], bounds[3]});
  int m = 0;
  for (int i = 0; i < n; i++) {
    if (skip[i]) continue;  // isBad() or IsInKeyFrame(pKF)
    const vsg::ProjectOut o = vsg::project_keyframe_point(*pose, kf, world_pos + 3 * (size_t)i, normal + 3 * (size_t)i,
                                                          min_dist[i], max_dist[i]);
    if (!o.valid) continue;
    index[m] = i, u[m] = o.u, v[m] = o.v, ur[m] = o.ur, level[m] = o.level;
    radius[m] = vsg::fmul(th, scale_factors[o.level]);
    memcpy(q_desc + 32 * (size_t)m, desc + 32 * (size_t)i, 32);
    m++;
  }
  return m;
}
