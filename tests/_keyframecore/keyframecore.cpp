// Host build of the per-point loop of Fuse x2 and SearchByProjection(pKF, Scw, ...) (vsg_project.h:
// project_keyframe_point), for tests/test_keyframe_projection_reference.py: the same source k_project_points compiles,
// against the NumPy restatement.
#include "vsg_project.h"

extern "C" {

// vsg::project_keyframe_point for n points; bounds = the FRAME's minX, minY, maxX, maxY (floats: the KeyFrame's truncated
// ones are derived as the library derives them); skip == nullptr: none
void kc_project_keyframe(const vsg_frame_pose *pose, const float *bounds, int n, const float *world_pos,
                         const float *normal, const float *min_dist, const float *max_dist, const uint8_t *skip,
                         uint8_t *valid, float *u, float *v, float *ur, int32_t *level) {
  const vsg::ImageBounds kf = vsg::keyframe_bounds({bounds[0], bounds[2], bounds[1], bounds[3]});
  for (int i = 0; i < n; i++) {
    vsg::ProjectOut o = {0, 0.0f, 0.0f, 0.0f, 0};
    if (!(skip && skip[i]))
      o = vsg::project_keyframe_point(*pose, kf, world_pos + 3 * i, normal + 3 * i, min_dist[i], max_dist[i]);
    valid[i] = (uint8_t)o.valid, u[i] = o.u, v[i] = o.v, ur[i] = o.ur, level[i] = o.level;
  }
}

// the truncated bounds alone: out = minX, minY, maxX, maxY
void kc_keyframe_bounds(const float *bounds, float *out) {
  const vsg::ImageBounds kf = vsg::keyframe_bounds({bounds[0], bounds[2], bounds[1], bounds[3]});
  out[0] = kf.minX, out[1] = kf.minY, out[2] = kf.maxX, out[3] = kf.maxY;
}
}
